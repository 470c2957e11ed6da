/* bayeformers_amd_spec.h — the speculative-decoding entry of the C-ABI (sample_generate(speculative=...)).  Included by
 * bayeformers_amd.h (include that one): the same conventions, the same library, the same BF_VERSION; bound by
 * bayeformers_amd/_C.py as SPEC_SYMBOLS.  An addition only: nothing bayeformers_amd.h declares changed with it.
 */
#ifndef BAYEFORMERS_AMD_SPEC_H
#define BAYEFORMERS_AMD_SPEC_H

#include "bayeformers_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- speculative decoding: the epilogue of one draft-and-verify iteration ---------------------------------------------
 * sample_generate(speculative = gamma) drafts gamma tokens per row with the posterior-mean weights and scores them under
 * the S pinned draws in one forward of gamma + 1 positions per row (the last kept token, then the drafts).  This entry
 * is what bf_generate_step is to the one-token step: one launch, one workgroup, no host synchronisation, capturable,
 * plain vector stores only.  With t = d_state[0] (int64[2] {step, 0}; the second word is left alone):
 *   inputs   d_argmax [B][gamma + 1]   the model-average argmax of each verified position (bf_mc_predictive_finish),
 *            d_draft [B][gamma]        the drafted tokens; position j of a row scores draft j,
 *            d_probs [B * (gamma + 1)][V] fp32 and the three entropies [B * (gamma + 1)], row b * (gamma + 1) + j.
 *   a_b  = the number of leading j with d_draft[b][j] == d_argmax[b][j];
 *   a    = the minimum of a_b over the rows not finished when the launch starts (every row, without eos_token_id; gamma
 *          when none is left), clipped to room = min(gamma, max_new_tokens - t - 1): all rows advance together, and
 *          t + a + 1 <= max_new_tokens.
 *   Row b receives a + 1 tokens at t .. t + a: its drafts 0 .. a - 1, then d_argmax[b][a] — the correction for the row
 *   that set the minimum, the continuation for the others, the model average's greedy token either way.  The eos /
 *   pad / finished / lengths rules are bf_generate_step's, position by position: a row finished before a position
 *   emits pad_token_id there with zero statistics and its length stops; emitting eos_token_id finishes it from the next
 *   position on.  Per kept position d_stats [4][B][max_new_tokens] gets that position's three entropies and the
 *   probability of the token written (0 for a token outside [0, V)).
 *   Writes, besides d_sequences, d_stats, d_finished and d_lengths: the next iteration's first verified token into
 *   column 0 of d_verify_ids [S * B][gamma + 1] (sample-major); d_draft_ids [B][2] = {the token in front of it, it} —
 *   the two tokens the next iteration's first draft step feeds (with a = 0 the first is the token this iteration's
 *   d_verify_ids held in column 0, read from sample 0's rows); a + 1 added to every element of d_verify_positions
 *   [S * B][gamma + 1] and d_draft_positions [B][gamma + 1] (each nullable); d_state[0] += a + 1; *d_rewind = gamma - a,
 *   what both caches' fill pointers go back by; d_speculation int64[3] += {1, room, a} — verify steps, drafts proposed
 *   (those that had room before max_new_tokens), drafts accepted.
 *   A launch at t >= max_new_tokens writes *d_rewind = gamma + 1 (the iteration's forwards advanced both fills by that)
 *   and nothing else.  gamma >= 1, B * (gamma + 1) <= 16, int64 arguments 8-byte aligned, seq_stride >= T0 +
 *   max_new_tokens; eos_token_id < 0: none (d_finished may then be NULL). */
int bf_spec_accept(const int64_t* d_argmax, const int64_t* d_draft, const float* d_probs,
                   const float* d_predictive_entropy, const float* d_expected_entropy, const float* d_mutual_information,
                   int64_t B, int64_t gamma, int64_t V, int S, int64_t* d_state, int64_t max_new_tokens,
                   int64_t* d_sequences, int64_t seq_stride, int64_t T0, float* d_stats, uint8_t* d_finished,
                   int64_t* d_lengths, int64_t* d_verify_ids, int64_t* d_verify_positions, int64_t* d_draft_ids,
                   int64_t* d_draft_positions, int64_t* d_rewind, int64_t* d_speculation, int64_t eos_token_id,
                   int64_t pad_token_id, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BAYEFORMERS_AMD_SPEC_H */
