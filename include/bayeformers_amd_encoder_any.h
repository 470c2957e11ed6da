/* bayeformers_amd_encoder_any.h — the encoder attention entries for any sequence length T >= 1 (head size 64, bf16 / fp16).
 * Includes bayeformers_amd.h: the same conventions, the same library, the same BF_VERSION; bound by bayeformers_amd/_C.py as
 * ENCODER_ANY_SYMBOLS.  Additions only: nothing bayeformers_amd.h declares changed with them.
 *
 * Each entry takes the arguments of its sibling in bayeformers_amd.h (bf_attention_fwd, _fwd_rows, _fwd_dropout,
 * bf_attention_bwd, _bwd_dropout) and computes the same function; with Tp = 128 * ceil(T / 128):
 *   * T % 128 == 0: the sibling's own checks, kernels and bits (T = 128 backward: the one-tile kernel);
 *   * otherwise the tail instantiations of those kernels, over ceil(T / 128) tiles.  Rows of q / k / v / out / dout past
 *     T - 1 are never read (a tile's missing rows re-read row T - 1 and carry no weight); keys >= T have probability
 *     exactly 0; queries >= T store nothing — no out, lse, delta, dq or keep word — and keys >= T no dk / dv.  The rows < T
 *     of the forward are bit for bit those of the sibling on a sequence padded to Tp whose pad keys are masked with -inf.
 *     d_mask ([B][T] fp32), d_lse and d_delta ([B][H][T] fp32) need 4-byte alignment only (they are read 4 bytes at a
 *     time: a row starts at a multiple of T floats); every other pointer 16 bytes, token_stride a multiple of 8 elements.
 *   * dropout: the keep words are [B][H][T][Tp / 32] (word (b, h, q, tile, lg), bit c*8 + e*4 + j as in the sibling), the
 *     group of probability (b, h, q, key) is ((((b*H + h)*T + q) * (Tp/32)) + (key/128)*4 + c) * 4 + lg + first_group; a
 *     caller that shards samples passes first_group = first sample * (sequences per sample) * H * T * (Tp/32) * 4.  Bits
 *     drawn for keys >= T are meaningless and unread.
 *   * a fully masked query gives out = 0 and lse = +inf, as in the siblings.
 * The column-sum fold (bf_attention_bwd_colsum) stays a T = 128 entry.
 * Asynchronous on `stream`, no allocation, no synchronisation (capturable).  Return 0, or 1 with bf_last_error() set,
 * before any launch. */
#ifndef BAYEFORMERS_AMD_ENCODER_ANY_H
#define BAYEFORMERS_AMD_ENCODER_ANY_H

#include "bayeformers_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bf_attention_fwd at any T >= 1. */
int bf_attention_fwd_any(const void* d_q, const void* d_k, const void* d_v, const float* d_mask /* nullable */,
                         const uint8_t* d_mask_off /* nullable */, void* d_out, float* d_lse /* nullable */, int dtype, int B,
                         int T, int H, int head_dim, int64_t token_stride, float scaling, void* stream);

/* bf_attention_fwd_dropout at any T >= 1; d_keep_bits (nullable): [B][H][T][Tp / 32]. */
int bf_attention_fwd_any_dropout(const void* d_q, const void* d_k, const void* d_v, const float* d_mask /* nullable */,
                                 const uint8_t* d_mask_off /* nullable */, void* d_out, float* d_lse /* nullable */, int dtype,
                                 int B, int T, int H, int head_dim, int64_t token_stride, float scaling, float p_drop,
                                 uint64_t seed, uint32_t call, uint32_t site, uint64_t first_group,
                                 uint32_t* d_keep_bits /* nullable */, const uint32_t* d_call /* nullable */, void* stream);

/* bf_attention_fwd_rows at any T >= 1: queries 0 .. q_rows - 1 (1 .. 16, q_rows <= T) against all T keys, d_out the compact
 * [B][q_rows][H][64]; bit for bit the first rows of bf_attention_fwd_any. */
int bf_attention_fwd_any_rows(const void* d_q, const void* d_k, const void* d_v, const float* d_mask /* nullable */,
                              const uint8_t* d_mask_off /* nullable */, void* d_out, int dtype, int B, int T, int H,
                              int head_dim, int64_t token_stride, int q_rows, float scaling, void* stream);

/* bf_attention_bwd at any T >= 1 (T % 128 != 0: the dq kernel, then the dk/dv kernel that reads its delta). */
int bf_attention_bwd_any(const void* d_q, const void* d_k, const void* d_v, const float* d_mask /* nullable */,
                         const uint8_t* d_mask_off /* nullable */, const void* d_out, const void* d_dout, const float* d_lse,
                         float* d_delta, void* d_dq, void* d_dk, void* d_dv, int dtype, int B, int T, int H, int head_dim,
                         int64_t token_stride, float scaling, void* stream);

/* bf_attention_bwd_dropout at any T >= 1; d_keep_bits: what bf_attention_fwd_any_dropout stored. */
int bf_attention_bwd_any_dropout(const void* d_q, const void* d_k, const void* d_v, const float* d_mask /* nullable */,
                                 const uint8_t* d_mask_off /* nullable */, const void* d_out, const void* d_dout,
                                 const float* d_lse, float* d_delta, void* d_dq, void* d_dk, void* d_dv, int dtype, int B,
                                 int T, int H, int head_dim, int64_t token_stride, float scaling, float p_drop,
                                 const uint32_t* d_keep_bits, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BAYEFORMERS_AMD_ENCODER_ANY_H */
