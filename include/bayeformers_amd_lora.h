/* bayeformers_amd_lora.h — the Bayesian low-rank adapter entries of the C-ABI (bnn.LoRALinear, to_bayesian_lora).  Included
 * by bayeformers_amd.h (include that one): the same conventions, the same library, the same BF_VERSION; bound by
 * bayeformers_amd/_C.py as LORA_SYMBOLS.  Additions only: nothing bayeformers_amd.h declares changed with them.
 */
#ifndef BAYEFORMERS_AMD_LORA_H
#define BAYEFORMERS_AMD_LORA_H

#include "bayeformers_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the layer these entries serve ---------------------------------------------------------------------------------
 * A frozen base projection W0 [N][K] (+ b0) with a rank-r adapter whose A factor is Gaussian (the BLoB formulation) and
 * whose B factor is a plain fp32 parameter.  For S Monte-Carlo samples, x sample-major [S][M][K], scale = alpha / r:
 *   A_s  = mu_A + softplus(rho_A) * eps(seed, sample_base + s, stream 2*layer_id, e)          [r][K]   (bf_sample_logprob)
 *   h[s] = x[s] A_s^T                                                                         [M][r]
 *   y[s] = x[s] W0^T + b0 + scale * h[s] B^T                                                  [M][N]
 * and, with eps a constant and the log-probs detached (the reference's graph),
 *   g[s]  = dy[s] B                                                                           [M][r]
 *   dx[s] = dy[s] W0 + scale * g[s] A_s
 *   dA_s  = scale * g[s]^T x[s]          -> dmu_A = sum_s dA_s,  drho_A = (sum_s dA_s o eps_s) o softplus'(rho_A)
 *   dB    = scale * sum_s dy[s]^T h[s]
 * The base products x W0^T and dy W0 are the caller's (bf_gemm_nt / bf_gemm_nt_skinny with S = 1, bf_gemm_nn): these entries
 * add the rank-r terms IN PLACE on their outputs.  A_s is sampled by bf_sample_logprob into the compute dtype.
 *
 * Supported class, both entries: dtype BF_DT_BF16 or BF_DT_F16 (operands and MFMA type; fp32 accumulation), K % 8 == 0,
 * N % 8 == 0, r % 8 == 0 with 8 <= r <= 64, S >= 1, M >= 1, every operand contiguous and 16-byte aligned.  Anything else
 * returns 1 with bf_last_error() naming the violated condition, before any launch.  The entries are asynchronous on
 * `stream`, allocate nothing, never synchronise (capturable) and use no floating-point atomics: every sum runs in a fixed
 * order, so two calls on the same inputs give the same bits. */

/* h = x A_s^T rounded to `dtype` and stored ([S][M][r]: the backward needs it), then y += scale * h B^T in place, the sum
 * formed in fp32 before the one rounding of y.  d_b is the fp32 master [N][r], rounded to `dtype` in registers.
 * Two launches, both on v_mfma_f32_16x16x32 (r zero-padded in registers to the instruction's k): the first forms h, one
 * workgroup per 16 rows of one sample with K dealt to its four waves, whose fp32 partial products are added in wave order;
 * the second walks y, one workgroup per 64-row tile and column range, 16 bytes of a row per lane, reading h and B through
 * L2.  (A single launch that kept the h tile in LDS was measured first and lost to this form at every size: its one
 * workgroup per row tile left the long K loop without loads in flight; profiles/bayesian_lora.md.)  x is read once, y is
 * read and written once.  d_y may be NULL (only h is wanted).  The workspace is not used today
 * (bf_lora_fwd_workspace_bytes = 0; d_workspace may be NULL). */
size_t bf_lora_fwd_workspace_bytes(int S, int M, int N, int K, int r, int dtype);
int bf_lora_fwd(const void* d_x, const void* d_a_s, const float* d_b, void* d_y /* in/out, nullable */, void* d_h /* out */,
                float scale, int dtype, int S, int M, int N, int K, int r, void* d_workspace, size_t workspace_bytes,
                void* stream);

/* g = dy B rounded to `dtype`, then dx += scale * g A_s in place (d_dx holds dy W0; NULL = not needed),
 * d_da[s] = scale * g[s]^T x[s] ([S][r][K] fp32, written) and d_db = scale * sum_s dy[s]^T h[s] ([N][r] fp32, written; NULL =
 * not needed).  d_h is what bf_lora_fwd stored.  The contractions over rows (M for dA_s, S*M for dB) are cut into chunks
 * that run on workgroups of their own and leave fp32 partial products in the workspace; a second launch adds them in chunk
 * order.  The workspace (bf_lora_bwd_workspace_bytes, 16-byte aligned) also holds B^T and A_s^T in `dtype` and g. */
size_t bf_lora_bwd_workspace_bytes(int S, int M, int N, int K, int r, int dtype);
int bf_lora_bwd(const void* d_x, const void* d_dy, const void* d_a_s, const float* d_b, const void* d_h,
                void* d_dx /* in/out, nullable */, float* d_da, float* d_db /* nullable */, float scale, int dtype, int S,
                int M, int N, int K, int r, void* d_workspace, size_t workspace_bytes, void* stream);

/* dmu_A = sum_s dA_s, drho_A = (sum_s dA_s o eps_s) o softplus'(rho_A): the reduction bf_linear_bwd ends with, on the
 * d_da that bf_lora_bwd wrote (n = r*K scalars per sample).  eps is regenerated from (seed, sample_base + s, stream_id)
 * plus the device-resident sample counter when one is set.  d_dmu may be NULL (frozen mean). */
int bf_lora_reduce_da(const float* d_da, const float* d_rho, uint64_t n, int S, uint64_t seed, uint32_t sample_base,
                      uint32_t stream_id, float* d_dmu, float* d_drho, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BAYEFORMERS_AMD_LORA_H */
