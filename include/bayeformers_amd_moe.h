/* bayeformers_amd_moe.h — the Bayesian mixture-of-experts entries of the C-ABI (bnn.Experts, to_bayesian(experts=True)).
 * Included by bayeformers_amd.h (include that one): the same conventions, the same library, the same BF_VERSION; bound by
 * bayeformers_amd/_C.py as MOE_SYMBOLS.  Additions only: nothing bayeformers_amd.h declares changed with them.
 */
#ifndef BAYEFORMERS_AMD_MOE_H
#define BAYEFORMERS_AMD_MOE_H

#include "bayeformers_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the layer these entries serve ---------------------------------------------------------------------------------
 * E gated experts with Gaussian posteriors on both weight tensors, gate_up [E][2I][H] and down [E][H][I].  For S Monte-Carlo
 * samples the rows of x [R][H] are sample-major: row r belongs to sample s = r / M, M = R / S, and meets that sample's draw
 * w_gu[s] / w_d[s] (bf_sample_logprob into the compute dtype, [S][E][2I][H] and [S][E][H][I]).  A router gives every row k
 * experts, top_k_index [R][k] (int64), and k weights.  A SLOT is one (row, j) pair, numbered r * k + j; its GROUP is
 * g = s * E + top_k_index[r][j], one of S * E weight matrices.
 *   h[slot]  = silu(x[r] Wg^T) * (x[r] Wu^T),   Wg = w_gu[s][e][0 .. I-1], Wu = w_gu[s][e][I .. 2I-1]          [I]
 *   y[slot]  = h[slot] w_d[s][e]^T                                                                              [H] fp32
 *   out[r]   = sum_j top_k_weights[r][j] * y[r * k + j]        (j = 0, 1, ... in this order, fp32, rounded once)
 * An index equal to E is a DROPPED slot (the framework's expert-parallel sentinel): it is in no group, its h and y rows are
 * never written and it adds nothing to out.  Any other index outside 0 .. E-1 is undefined input; the entries treat it as
 * dropped too (no address is ever formed from it), but nothing is promised about it.
 *
 * Supported class: dtype BF_DT_BF16 or BF_DT_F16 (operands and MFMA type, fp32 accumulation), H % 8 == 0, I % 8 == 0 (tails
 * of the contraction and of the features are zero-filled and masked), 1 <= k <= BF_MOE_MAX_TOPK, S * E <= BF_MOE_MAX_GROUPS,
 * R % S == 0, R * k < 2^31, every operand contiguous and 16-byte aligned.  Anything else returns 1 with bf_last_error()
 * naming the entry and the violated condition, before any launch.  The entries are asynchronous on `stream`, allocate
 * nothing, read nothing back to the host (capturable) and use no atomics of any kind: every output element is written by one
 * thread and every sum runs in a fixed order, so two calls on the same inputs give the same bits. */
#define BF_MOE_TILE_ROWS 16    /* BM: rows of a tile = one v_mfma_f32_16x16x32 row block; a decode step's groups of one or
                                  two rows pad no more than that and mostly stream their weights */
#define BF_MOE_MAX_TOPK 16     /* cap on k */
#define BF_MOE_MAX_GROUPS 4096 /* cap on S * E */

/* Tiles the GEMM entries are launched with for R rows of k slots in G = S * E groups: R*k / BM + min(G, R*k), a bound
 * on sum_g ceil(count_g / BM) that needs no data.  Tiles past the real count have 0 live rows and exit at once. */
size_t bf_moe_max_tiles(int S, int E, int R, int k);

/* Lay the slots out by group on the device.  d_top_k_index [R][k] int64.
 *   d_offsets [S*E + 1] int32: group g owns positions offsets[g] .. offsets[g+1]-1 of d_slots; offsets[S*E] = live slots
 *   d_slots   [R*k]     int32: slot numbers sorted by group, in (row, j) order inside a group (stable: the same input gives
 *                              the same list); positions from offsets[S*E] on are not written
 *   d_tiles   [bf_moe_max_tiles][3] int32: {group, first position in d_slots, live rows (1 .. BM)} per tile, groups in
 *                              order; {0, 0, 0} for the surplus tiles
 * Three launches: a wave per (sample, expert) counts its slots (ballot over 64 slots a step), one workgroup scans the
 * counts and writes offsets and the tile table, and the first kernel runs again to write the slots.  The workspace
 * (bf_moe_route_workspace_bytes, 16-byte aligned) holds the counts. */
size_t bf_moe_route_workspace_bytes(int S, int E, int R, int k);
int bf_moe_route(const long long* d_top_k_index, int* d_offsets, int* d_slots, int* d_tiles, int S, int E, int R, int k,
                 void* d_workspace, size_t workspace_bytes, void* stream);

/* h[slot] = silu(gate) * up for every live slot, [R*k][I] of `dtype`: per tile the rows of x are gathered through d_slots
 * (row = slot / k) and multiplied by the group's w_gu [2I][H]; the activation runs on the fp32 accumulators and h is rounded
 * once.  grid = (bf_moe_max_tiles, ceil(I / 64)): a wave owns 16 features of gate and the same 16 of up.  Rows of a tile
 * beyond its live count are multiplied as zeros and never stored.  No workspace (bf_moe_gate_up_workspace_bytes = 0). */
size_t bf_moe_gate_up_workspace_bytes(int S, int E, int R, int k, int H, int I, int dtype);
int bf_moe_gate_up(const void* d_x, const void* d_w_gu, const int* d_slots, const int* d_tiles, void* d_h, int dtype, int S,
                   int E, int R, int k, int H, int I, void* d_workspace, size_t workspace_bytes, void* stream);

/* y[slot] = h[slot] w_d[s][e]^T for every live slot, fp32 [R*k][H] = [R][k][H]: each result at the slot's own place. */
size_t bf_moe_down_workspace_bytes(int S, int E, int R, int k, int H, int I, int dtype);
int bf_moe_down(const void* d_h, const void* d_w_d, const int* d_slots, const int* d_tiles, float* d_y, int dtype, int S,
                int E, int R, int k, int H, int I, void* d_workspace, size_t workspace_bytes, void* stream);

/* out[r] = sum_j weights[r][j] * y[r][j] over the slots with 0 <= index < E, [R][H] of `dtype`.  d_top_k_weights [R][k] of
 * `weights_dtype` (BF_DT_F32, or `dtype`).  A launch of its own: a row's k slots lie in k different tiles of bf_moe_down. */
size_t bf_moe_combine_workspace_bytes(int R, int k, int H);
int bf_moe_combine(const float* d_y, const long long* d_top_k_index, const void* d_top_k_weights, int weights_dtype,
                   void* d_out, int dtype, int E, int R, int k, int H, void* d_workspace, size_t workspace_bytes,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BAYEFORMERS_AMD_MOE_H */
