/* bayeformers_amd_lrt.h — the local reparameterisation entries of the C-ABI (bnn.Linear with `local = True`,
 * bayeformers_amd.local_reparameterization; Kingma, Salimans, Welling 2015).  Included by bayeformers_amd.h (include that
 * one): the same conventions, the same library, the same BF_VERSION; bound by bayeformers_amd/_C.py as LRT_SYMBOLS.
 * Additions only: nothing bayeformers_amd.h declares changed with them.
 */
#ifndef BAYEFORMERS_AMD_LRT_H
#define BAYEFORMERS_AMD_LRT_H

#include "bayeformers_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the layer these entries serve ---------------------------------------------------------------------------------
 * For a factorised Gaussian posterior the pre-activation of every row is itself Gaussian, so the layer samples its outputs
 * instead of its weights.  For S Monte-Carlo samples, x sample-major [S][M][K] with R = S*M rows, sigma = softplus(rho):
 *   m = x mu^T + mu_b            v = x^2 (sigma^2)^T + sigma_b^2            y[s][i][n] = act(m + sqrt(v) * zeta)
 * zeta of element e = i*N + n of sample s is component e & 3 of group e >> 2 of
 *   Philox4x32-7(counter {lo32(g), sample_base + s (+ the device sample counter when set), BF_LRT_STREAM | layer_id, hi32(g)},
 *                key = seed),      BF_LRT_STREAM = 0x20000000 (csrc/bf_philox.h),
 * Box-Muller as for eps: a function of the GLOBAL sample index.  The bias has no draw of its own.
 * With zeta a constant and g the gradient at the pre-activation (dy, times act'(pre) under a fused activation):
 *   dm = g        dv = g * zeta / (2 sqrt(v)), 0 where v == 0
 *   dx = dm mu + 2 x o (dv sigma^2)        dmu = dm^T x        dsigma^2 = dv^T x^2        drho = dsigma^2 * 2 sigma sigmoid(rho)
 *   dmu_b = colsum(dm)                      drho_b = colsum(dv) * 2 sigma_b sigmoid(rho_b)
 *
 * The matrix products are the caller's, on the GEMM entries of bayeformers_amd.h:
 *   [m; v]   = bf_gemm_nt_act on [x; x^2] and [mu; sigma^2] with the bias pair [mu_b; sigma_b^2], the sample axis used as the
 *              pair axis (S = 2, M = R) — or two S = 1 launches.  y_dtype BF_DT_F32: m and v leave the GEMM in fp32, so the
 *              small v of a MOPED posterior is not rounded before its square root.
 *   [a; b]   = bf_gemm_nn on [dm; dv] and [mu; sigma^2] (16-bit out), dx = a + 2 x o b (bf_lrt_dx)
 *   [dmu; dsigma^2] = bf_gemm_tn with batch 2 on [dm; dv] and [x; x^2] (fp32 out): ONE [2][N][K] contraction over all R rows,
 *              whatever S is.  It wants R % 64 == 0: the operands may be padded to R_pad rows, which the entries below
 *              write as zeros.
 *
 * Supported class: dtype BF_DT_BF16 (fp16: x^2 overflows above |x| = 256 and a MOPED sigma^2 underflows), K % 8 == 0,
 * N % 8 == 0, S*M < 2^31 - 64, every operand contiguous and 16-byte aligned.  Anything else returns 1 with bf_last_error()
 * naming the violated condition, before any launch.  The entries are asynchronous on `stream`, allocate nothing, never
 * synchronise (capturable) and use no floating-point atomics: every sum runs in a fixed order, so two calls on the same
 * inputs give the same bits.  A lane moves 16 bytes of each 16-bit tensor: 8 consecutive elements of one row. */

/* The GEMM operands from the fp32 masters: d_w2 [2][N][K] bf16 = [mu; sigma^2] and d_b2 [2][N] fp32 = [mu_b; sigma_b^2], each
 * one rounding of the fp32 value (softplus in its stable form: sigma^2 stays finite and non-zero from rho = -30 to rho = 20
 * and beyond).  No bias: d_mu_b, d_rho_b and d_b2 all NULL. */
int bf_lrt_operands(const float* d_mu, const float* d_rho, const float* d_mu_b /* nullable */,
                    const float* d_rho_b /* nullable */, void* d_w2, float* d_b2 /* nullable */, int dtype, int N, int K,
                    void* stream);

/* d_xx [2][R_pad][K] from x [R][K]: slab 1 = x^2 (squared in fp32, rounded once), slab 0 = x when pair != 0 (untouched
 * otherwise: the two-launch form reads x where it lies).  Rows R .. R_pad of every written slab are zeros, R <= R_pad <=
 * R + 64. */
int bf_lrt_square(const void* d_x, void* d_xx, int dtype, int R, int R_pad, int K, int pair, void* stream);

/* y = act(m + sqrt(v) * zeta) from the fp32 moments d_m, d_v [S*M][N]; zeta is drawn in registers (two Philox groups per
 * lane, one sample index).  act = BF_ACT_GELU applies the exact erf-GELU to the unrounded pre-activation.  d_pre (nullable):
 * the pre-activation in `dtype`, what the backward of a fused activation reads; d_sd (nullable): sqrt(v) in `dtype`, what
 * bf_lrt_grad_prepare reads (a negative v, which only rounding can produce, counts as 0). */
int bf_lrt_combine(const float* d_m, const float* d_v, void* d_y, void* d_pre /* nullable */, void* d_sd /* nullable */,
                   int dtype, int S, int M, int N, int act, uint64_t seed, uint32_t sample_base, uint32_t layer_id,
                   void* stream);

/* zeta alone, d_out [S][M*N] fp32, for any M and N (honours the device sample counter, which bf_philox_normal does not):
 * what the framework composite of the layer and the tests read. */
int bf_lrt_zeta(float* d_out, int S, int M, int N, uint64_t seed, uint32_t sample_base, uint32_t layer_id, void* stream);

/* d_dmdv [2][R_pad][N] = [dm; dv] in `dtype` from dy [S*M][N], sqrt(v) as bf_lrt_combine stored it and zeta regenerated
 * from the counter; under act = BF_ACT_GELU, g = dy * gelu'(pre) with d_pre as bf_lrt_combine stored it (d_pre is given
 * exactly when act != BF_ACT_NONE).  dv is exactly 0 where sqrt(v) == 0; rows S*M .. R_pad are zeros.  d_colsum [2][N] fp32:
 * the column sums of dm and dv (of their fp32 values, before the rounding to `dtype`), formed per chunk of 256 rows in the
 * same pass and added in chunk order by a second launch.  Workspace: bf_lrt_grad_prepare_workspace_bytes, 16-byte aligned. */
size_t bf_lrt_grad_prepare_workspace_bytes(int R_pad, int N);
int bf_lrt_grad_prepare(const void* d_dy, const void* d_pre /* nullable */, const void* d_sd, void* d_dmdv, float* d_colsum,
                        int dtype, int S, int M, int R_pad, int N, int act, uint64_t seed, uint32_t sample_base,
                        uint32_t layer_id, void* d_workspace, size_t workspace_bytes, void* stream);

/* dx [R][K] = a + 2 x o b, the sum in fp32 before the one rounding; a = d_ab, b = d_ab + slab elements (the two slabs of
 * the NN product, slab >= R*K). */
int bf_lrt_dx(const void* d_ab, int64_t slab, const void* d_x, void* d_dx, int dtype, int R, int K, void* stream);

/* d_drho[e] = d_dsig2[e] * 2 softplus(rho[e]) sigmoid(rho[e]) for e < n, n % 4 == 0: the weight's [N*K] and the bias's [N]. */
int bf_lrt_drho(const float* d_dsig2, const float* d_rho, float* d_drho, uint64_t n, void* stream);

/* bf_sample_logprob's log-probs with no sample written, evaluated by the kernel instantiation that writes `like_dtype`
 * weights (a second tensor: fp32): {log_prior, log_q} per sample with the BITS of the per-layer forward that draws those
 * weights (bf_linear_fwd at compute dtype `like_dtype`) — what kl="sampled" puts into a local layer's slot.  (Without an
 * output bf_sample_logprob runs an instantiation of its own, whose fp32 terms may differ in the last bit.)  Arguments and
 * workspace as bf_sample_logprob (bf_sample_logprob_workspace_bytes); every d_sample_out must be NULL. */
int bf_sample_logprob_like(const bf_tensor_t* tensors, int n_tensors, int S, uint64_t seed, uint32_t sample_base,
                           double* d_logprob_out, void* d_workspace, size_t workspace_bytes, int like_dtype, void* stream);

/* The closed-form expectations of one tensor's log-probs under a Gaussian prior N(mu_p, softplus(rho_p)), d_out[2] fp64:
 *   d_out[0] = E_q log p = -sum(log sigma_p + 1/2 log 2 pi + (sigma^2 + (mu - mu_p)^2) / (2 sigma_p^2))
 *   d_out[1] = E_q log q = -sum(log sigma + 1/2 log 2 pi + 1/2)
 * One pass, fp64 arithmetic and accumulation: a thread adds its elements in index order, a block's threads meet in a fixed
 * tree, and a second launch adds the block partials in block order.  Workspace: bf_kl_gaussian_workspace_bytes(). */
size_t bf_kl_gaussian_workspace_bytes(void);
int bf_kl_gaussian(const float* d_mu, const float* d_rho, const float* d_prior_mu, const float* d_prior_rho, uint64_t n,
                   double* d_out, void* d_workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BAYEFORMERS_AMD_LRT_H */
