/* bayeformers_amd_ring.h — the ring-buffer KV-cache entries of the C-ABI (sample_generate(sliding_cache="ring")).  Included
 * by bayeformers_amd.h (include that one): the same conventions, the same library, the same BF_VERSION; bound by
 * bayeformers_amd/_C.py as RING_SYMBOLS.  Additions only: nothing bayeformers_amd.h declares changed with them.
 */
#ifndef BAYEFORMERS_AMD_RING_H
#define BAYEFORMERS_AMD_RING_H

#include "bayeformers_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the ring -----------------------------------------------------------------------------------------------------
 * A sliding-window layer with window W never shows a query more than W keys, so its cache need not hold the whole
 * capacity: it holds C = ring_slots rows per (sequence n, K/V head g), and the key with sequence index j lives in row
 * j % C.  A step that appends Tq rows at fill L reads the keys [L - W + 1, L + Tq) at most: W + Tq - 1 <= C of them, so none
 * was overwritten by the step's own rows.  The fill L is a device int64 that counts every appended row and never wraps.
 * All entries are asynchronous on `stream`, allocate nothing and never synchronise (capturable); they return 0, or 1
 * with bf_last_error() set, before any launch. */

/* Append the new K and V rows of a forward.  d_k, d_v [N][Hkv][T][D] of `dtype` (BF_DT_BF16 or BF_DT_F16), each with its own
 * (batch, head, token) element strides k_stride[3] / v_stride[3] (host arrays; non-negative multiples of 8) and a contiguous
 * feature dimension; d_kc, d_vc [N][Hkv][ring_slots][D] of the same dtype, contiguous.  Row i of the call goes to row
 * (*d_pos + i) % ring_slots, d_pos a device int64 read by the kernel (the fill before this call).  Any T >= 1: of
 * T > ring_slots rows only the last ring_slots are written (the earlier ones' rows would be overwritten within the call),
 * so no row is written twice in a launch.  Every row index is a remainder by ring_slots: nothing outside the two buffers is
 * written whatever *d_pos holds (a negative value writes nothing).  D 64, 128 or 256, one launch for K and V.  d_k, d_v,
 * d_kc, d_vc 16-byte, d_pos 8-byte aligned. */
int bf_kv_ring_append(const void* d_k, const void* d_v, int dtype, const int64_t* k_stride, const int64_t* v_stride,
                      void* d_kc, void* d_vc, const int64_t* d_pos, int N, int Hkv, int T, int D, int ring_slots,
                      void* stream);

/* bf_kv_ring_append into an FP8 ring: bf_kv8_append's quantisation (bayeformers_amd_kv8.h: D e4m3fn bytes and one fp32
 * power-of-two scale per row; dtype must be BF_DT_BF16) with bf_kv_ring_append's placement.  d_kq, d_vq
 * [N][Hkv][ring_slots][D] bytes and d_k_scale, d_v_scale [N][Hkv][ring_slots] fp32 (4-byte aligned), contiguous. */
int bf_kv8_ring_append(const void* d_k, const void* d_v, int dtype, const int64_t* k_stride, const int64_t* v_stride,
                       void* d_kq, void* d_vq, float* d_k_scale, float* d_v_scale, const int64_t* d_pos, int N, int Hkv,
                       int T, int D, int ring_slots, void* stream);

/* bf_attention_decode_gqa_softcap with a window over a ring: shape->Tk is the LOGICAL capacity — it sets the grid, the key
 * split, the workspace (bf_attention_decode_workspace_bytes(shape), unchanged) and the width of d_mask [N][Tk], which
 * stays over sequence indices — while d_k and d_v hold ring_slots rows (the token stride of `shape` steps through them), key
 * j in row j % ring_slots.  d_kv_len (required: the fill L, a device int64) and the visibility test are those of
 * bf_attention_decode_gqa_len_window: query i has index L - Tq + i and sees the keys within `window` of it.
 * window >= 1 and window + Tq - 1 <= ring_slots are required; softcap 0 = none.  The result is bitwise that of the window
 * entry on the same keys held in sequence order in a cache of Tk rows. */
int bf_attention_decode_gqa_ring(const void* d_q, const void* d_k, const void* d_v, const float* d_mask /* nullable */,
                                 const uint8_t* d_mask_off /* nullable */, const int64_t* d_kv_len, void* d_out,
                                 void* d_workspace, int dtype, const bf_attn_decode_t* shape, int32_t ring_slots,
                                 int32_t window, float softcap, float scaling, void* stream);

/* The same on an FP8 ring (bf_attention_decode_gqa_kv8's arguments): d_kq, d_vq [..][ring_slots][D] bytes with strides in
 * bytes (multiples of 16), the scales contiguous [N][Hkv][ring_slots]; dtype must be BF_DT_BF16. */
int bf_attention_decode_gqa_ring_kv8(const void* d_q, const void* d_kq, const void* d_vq, const float* d_k_scale,
                                     const float* d_v_scale, const float* d_mask /* nullable */,
                                     const uint8_t* d_mask_off /* nullable */, const int64_t* d_kv_len, void* d_out,
                                     void* d_workspace, int dtype, const bf_attn_decode_t* shape, int32_t ring_slots,
                                     int32_t window, float softcap, float scaling, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BAYEFORMERS_AMD_RING_H */
