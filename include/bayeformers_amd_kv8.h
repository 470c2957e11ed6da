/* bayeformers_amd_kv8.h — the FP8 KV-cache entries of the C-ABI (sample_generate(kv_cache="fp8")).  Included by
 * bayeformers_amd.h (include that one): the same conventions, the same library, the same BF_VERSION; bound by
 * bayeformers_amd/_C.py as KV8_SYMBOLS.  Additions only: nothing bayeformers_amd.h declares changed with them.
 */
#ifndef BAYEFORMERS_AMD_KV8_H
#define BAYEFORMERS_AMD_KV8_H

#include "bayeformers_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- kv8 rows: the format -----------------------------------------------------------------------------------------
 * For each (sequence n, K/V head g, cache slot j) the K row and the V row x [D] (bf16) are each stored as the centred FP8
 * rows of bayeformers_amd_fp8.h with centre zero:
 *   a            = max_d |x|
 *   e            = the smallest integer with a * 2^-e <= 448 (that header's rule; 0 if a = 0; clamped to [-64, 64])
 *   scale[n][g][j] = 2^e                                                      fp32
 *   q[n][g][j][d]  = e4m3fn_rne(clamp(x * 2^-e, -448, 448))                   one byte, OCP E4M3 (finite-only, bias 7)
 * The dequantised value x^ = float(q) * scale is exact in bf16 (3 mantissa bits times a power of two), so only bf16 is
 * taken.  |x^ - x| <= 2^-4 |x| where |x| >= 2^-6 scale, <= 2^-10 scale below that, and scale <= a / 224.  A row pair is
 * 2 D + 8 bytes against 4 D in bf16.  Inputs are finite; inf and NaN are not specified.
 * All entries are asynchronous on `stream`, allocate nothing and never synchronise (capturable); they return 0, or 1
 * with bf_last_error() set, before any launch. */

/* Quantise the new K and V rows of a forward into the cache.  d_k, d_v [N][Hkv][Tq][D] bf16 (dtype must be BF_DT_BF16),
 * each with its own (batch, head, token) element strides k_stride[3] / v_stride[3] (host arrays; non-negative multiples
 * of 8) and a contiguous feature dimension; d_kq, d_vq [N][Hkv][capacity][D] bytes and d_k_scale, d_v_scale
 * [N][Hkv][capacity] fp32, contiguous.  Row i of the call goes to slot *d_pos + i, d_pos a device int64 read by the
 * kernel (the cache's fill before this call); a row whose slot is < 0 or >= capacity is skipped, so nothing outside the
 * four buffers is written whatever *d_pos holds.  Any Tq >= 1, D 64, 128 or 256, one launch for K and V.  d_k, d_v, d_kq,
 * d_vq 16-byte, the scales 4-byte, d_pos 8-byte aligned. */
int bf_kv8_append(const void* d_k, const void* d_v, int dtype, const int64_t* k_stride, const int64_t* v_stride, void* d_kq,
                  void* d_vq, float* d_k_scale, float* d_v_scale, const int64_t* d_pos, int N, int Hkv, int Tq, int D,
                  int capacity, void* stream);

/* x^ [rows][D] bf16 <- q [rows][D] bytes, scale [rows] fp32 (dtype must be BF_DT_BF16; D a multiple of 16; q and out
 * 16-byte aligned). */
int bf_kv8_dequantize(const void* d_q, const float* d_scale, void* d_out, int dtype, int64_t rows, int D, void* stream);

/* bf_attention_decode_gqa_softcap on an FP8 cache: (d_kq, d_vq, d_k_scale, d_v_scale) in place of (d_k, d_v); d_kv_len
 * nullable (the fill of a fixed-capacity cache), window 0 = none, softcap 0 = none.  The K / V strides of `shape` are in
 * bytes (= elements) and must be multiples of 16; the scales are contiguous [N][Hkv][Tk].  dtype (of q and out) must be
 * BF_DT_BF16.  The key split and the workspace are bf_attention_decode_workspace_bytes(shape)'s; the result is bitwise
 * that of the bf16 entry on the dequantised cache. */
int bf_attention_decode_gqa_kv8(const void* d_q, const void* d_kq, const void* d_vq, const float* d_k_scale,
                                const float* d_v_scale, const float* d_mask /* nullable */,
                                const uint8_t* d_mask_off /* nullable */, const int64_t* d_kv_len /* nullable */, void* d_out,
                                void* d_workspace, int dtype, const bf_attn_decode_t* shape, int32_t window, float softcap,
                                float scaling, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BAYEFORMERS_AMD_KV8_H */
