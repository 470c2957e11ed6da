/* bayeformers_amd_softcap.h — the soft-cap attention entries of the C-ABI.  Included by bayeformers_amd.h (include that
 * one): the same conventions, the same library, the same BF_VERSION; bound by bayeformers_amd/_C.py as SOFTCAP_SYMBOLS.
 * Additions only: nothing bayeformers_amd.h declares changed with them.
 */
#ifndef BAYEFORMERS_AMD_SOFTCAP_H
#define BAYEFORMERS_AMD_SOFTCAP_H

#include "bayeformers_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- soft-capped logits (Gemma 2) ---------------------------------------------------------------------------------
 * The causal entries of bayeformers_amd.h (bf_attention_fwd_gqa / bf_attention_bwd_gqa / bf_attention_decode_gqa and
 * their _window and _len siblings; shapes, strides, masks and workspaces are described there) with the attention
 * logits soft-capped before the mask and the softmax:
 *   s[i][j] = softcap * tanh(scaling q[i] . k[j] / softcap) + mask[j],   out[i] = sum_j softmax_j(s[i][j]) v[j]
 * — what HF Gemma2Attention asks of its attention function with softcap = config.attn_logit_softcapping (50.0;
 * transformers' models/gemma2/modeling_gemma2.py eager_attention_forward: `attn_weights / softcap`, `torch.tanh`,
 * `* softcap`, then `+ attention_mask`), between the Bayesian q/k/v_proj and o_proj layers to_bayesian converts
 * (/root/reference/bayeformers/convert.py).  `window` is the sliding window of the _window entries or 0 for none;
 * `softcap` must be finite and > 0.  Three entries for the eight plain / window ones: forward, backward (d_lse is the
 * log-sum of the capped scores, as the forward stores it; dS carries the factor 1 - tanh^2), and the decode step, whose
 * d_kv_len is NULL (shape->Tk keys, as bf_attention_decode_gqa) or the device scalar of bf_attention_decode_gqa_len
 * (shape->Tk the capacity), with the workspace of bf_attention_decode_workspace_bytes(shape).  Everything else — the
 * arguments, the key mask, the tail forms for any T, rows with no visible key (output 0, lse = +inf, zero gradients),
 * bitwise reproducibility — is the plain entry's.  Refused (1, bf_last_error() set): softcap not finite or <= 0,
 * window < 0, a shape with causal == 0, and whatever the plain entries refuse.  These run their own instantiations of
 * the kernels; the plain and window entries run the ones they always ran. */
int bf_attention_fwd_gqa_softcap(const void* d_q, const void* d_k, const void* d_v, const float* d_mask,
                                 const uint8_t* d_mask_off, void* d_out, float* d_lse, int dtype, const bf_attn_gqa_t* shape,
                                 int32_t window, float softcap, float scaling, void* stream);
int bf_attention_bwd_gqa_softcap(const void* d_q, const void* d_k, const void* d_v, const float* d_mask,
                                 const uint8_t* d_mask_off, const void* d_out, const void* d_dout, const float* d_lse,
                                 float* d_delta, void* d_dq, void* d_dk, void* d_dv, int dtype, const bf_attn_gqa_t* shape,
                                 int32_t window, float softcap, float scaling, void* stream);
int bf_attention_decode_gqa_softcap(const void* d_q, const void* d_k, const void* d_v, const float* d_mask,
                                    const uint8_t* d_mask_off, const int64_t* d_kv_len /* nullable */, void* d_out,
                                    void* d_workspace, int dtype, const bf_attn_decode_t* shape, int32_t window,
                                    float softcap, float scaling, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BAYEFORMERS_AMD_SOFTCAP_H */
