/* bayeformers_amd_packed.h — the banded causal attention entries of the C-ABI (packed sequences).  Included by
 * bayeformers_amd.h (include that one): the same conventions, the same library, the same BF_VERSION; bound by
 * bayeformers_amd/_C.py as PACKED_SYMBOLS.  Additions only: nothing bayeformers_amd.h declares changed with them.
 */
#ifndef BAYEFORMERS_AMD_PACKED_H
#define BAYEFORMERS_AMD_PACKED_H

#include "bayeformers_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- banded causal attention (packed sequences) -------------------------------------------------------------------
 * Padding-free fine-tuning lays several documents end to end in one batch row (position ids restart at each document,
 * no padding mask); a token attends to the earlier tokens of its own document only, within the sliding window where the
 * layer has one.  Both are one contract, banded causal attention: query i of sequence b sees key j iff
 *   lo[b][i] <= j <= i.
 * d_lo is [B][T] int32, non-decreasing along T, with 0 <= lo[b][i] <= i.  d_hi is the transposed bound, the last query
 * that sees key j: [B][T] int32, non-decreasing along T, with j <= hi[b][j] < T, and consistent with lo
 * (lo[b][i] <= j <= i  iff  j <= i <= hi[b][j]).  For packed documents with an optional window W:
 *   lo[i] = max(doc_start(i), i - W + 1),   hi[j] = min(doc_end(j), j + W - 1).
 * Every row sees at least itself, so no row is empty.  The forward and the dq kernel read d_lo, the dk/dv kernel d_hi.
 * The bounds are device arrays: that they are monotone, in range and consistent with each other is the CALLER'S
 * responsibility — the entries cannot check it.  (Bounds that are not give wrong results; the kernels clamp the tile
 * range they derive from them, so no row outside [0, T) is read or written.)
 * The shapes, strides, outputs (d_out [B][T][H][D], d_lse [B][H][T] in log2 units, nullable in the forward; d_delta,
 * d_dq, d_dk, d_dv as bf_attention_bwd_gqa), the tail forms for any T >= 1 and bitwise reproducibility are those of
 * bf_attention_fwd_gqa / bf_attention_bwd_gqa.  There is NO key-padding mask and no soft-cap.  With lo = 0 and
 * hi = T - 1 the results are bitwise those of the plain causal entries, and with the bounds of one document and a
 * window W those of the _window entries.  Refused (1, bf_last_error() set) before any launch: d_lo NULL, d_hi NULL
 * (backward), a shape with causal != 1, d_lo / d_hi not 4-byte aligned, and whatever the plain entries refuse.  These
 * run their own instantiations of the kernels; the other entries run the ones they always ran. */
int bf_attention_fwd_gqa_band(const void* d_q, const void* d_k, const void* d_v, const int32_t* d_lo, void* d_out,
                              float* d_lse /* nullable */, int dtype, const bf_attn_gqa_t* shape, float scaling,
                              void* stream);
int bf_attention_bwd_gqa_band(const void* d_q, const void* d_k, const void* d_v, const int32_t* d_lo, const int32_t* d_hi,
                              const void* d_out, const void* d_dout, const float* d_lse, float* d_delta, void* d_dq,
                              void* d_dk, void* d_dv, int dtype, const bf_attn_gqa_t* shape, float scaling, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BAYEFORMERS_AMD_PACKED_H */
