/* bayeformers_amd_chunk.h — the cached-chunk attention entries of the C-ABI (sample_generate(prefill_chunk=...)).  Includes
 * bayeformers_amd.h: the same conventions, the same library, the same BF_VERSION; bound by bayeformers_amd/_C.py as
 * CHUNK_SYMBOLS.  Additions only: nothing bayeformers_amd.h declares changed with them.
 */
#ifndef BAYEFORMERS_AMD_CHUNK_H
#define BAYEFORMERS_AMD_CHUNK_H

#include "bayeformers_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Causal grouped-query attention of a chunk of Tq new queries against Tk cached keys, bottom-right aligned; forward only
 * (no gradient, no dropout, no lse).  `shape` is bf_attention_decode_gqa's, with any Tq in 1 .. Tk: q element (n, h, i, d)
 * at n q_stride[0] + h q_stride[1] + i q_stride[2] + d, k / v likewise with g = h / (H / Hkv); head_dim 64, 128 or 256;
 * strides non-negative multiples of 8 elements, 16-byte aligned pointers; dtype BF_DT_BF16 or BF_DT_F16.
 *   L   = *d_kv_len clamped to [0, Tk] (a device int64, 8-byte aligned, read by the kernel: the fill of a fixed-capacity
 *         cache AFTER this call's rows were appended), or Tk when d_kv_len is NULL;
 *   p_i = L - Tq + i, the position of query i; a query with p_i < 0 sees nothing;
 *   query i sees the keys max(0, p_i - window + 1) .. p_i (window 0: 0 .. p_i) that d_mask leaves visible.
 * key_origin >= 0 is the index in its sequence of the cache's key 0: 0 for a cache that holds the sequence from its start,
 * the number of dropped keys for one that kept a sliding window's last keys only.  It moves no bound — positions stay
 * relative to L — but the kernel lays its key tiles on the sequence's tile grid (multiples of the tile from the sequence's
 * key 0, as bf_attention_fwd_gqa lays them), so a chunk's rows round as the same rows of a whole-sequence forward do.
 * Keys j >= L are never read (they may hold anything).  d_mask: additive fp32 [N][Tk] over the keys or NULL (4-byte
 * aligned), d_mask_off: NULL or a device byte, non-zero = the mask hides nothing.  softcap > 0: the score is
 * softcap * tanh(scaling q.k / softcap), capped before the mask and the -inf's, as in bf_attention_fwd_gqa_softcap;
 * 0: no cap.  d_out: [N][Tq][H][head_dim] contiguous; a query with no visible key gives 0.
 * One launch whose grid depends on the shape only; asynchronous on `stream`, no allocation, no synchronisation
 * (capturable: a captured launch replays correctly after *d_kv_len changed).  Returns 0, or 1 with bf_last_error() set,
 * before any launch: a NULL or misaligned pointer, head size, H % Hkv, Tq < 1, Tq > Tk, N or H above 65535, a stride
 * that is no multiple of 8, window < 0, key_origin < 0, softcap negative or not finite. */
int bf_attention_chunk_gqa(const void* d_q, const void* d_k, const void* d_v, const float* d_mask /* nullable */,
                           const uint8_t* d_mask_off /* nullable */, const int64_t* d_kv_len /* nullable */, void* d_out,
                           int dtype, const bf_attn_decode_t* shape, int32_t window, int32_t key_origin, float softcap,
                           float scaling, void* stream);

/* bf_attention_chunk_gqa on an FP8 cache (bayeformers_amd_kv8.h): (d_kq, d_vq, d_k_scale, d_v_scale) in place of
 * (d_k, d_v).  The K / V strides of `shape` are in bytes (= elements) and must be multiples of 16; the scales are
 * contiguous fp32 [N][Hkv][Tk], 4-byte aligned; rows and scales at or past L are never read.  dtype (of q and out) must be
 * BF_DT_BF16.  The rows are dequantised in registers; the result is bitwise that of bf_attention_chunk_gqa on the
 * dequantised cache. */
int bf_attention_chunk_gqa_kv8(const void* d_q, const void* d_kq, const void* d_vq, const float* d_k_scale,
                               const float* d_v_scale, const float* d_mask /* nullable */,
                               const uint8_t* d_mask_off /* nullable */, const int64_t* d_kv_len /* nullable */, void* d_out,
                               int dtype, const bf_attn_decode_t* shape, int32_t window, int32_t key_origin, float softcap,
                               float scaling, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BAYEFORMERS_AMD_CHUNK_H */
