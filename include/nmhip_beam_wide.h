/* libnmhip -- C ABI of the beam step for wide beams (17 to 64 hypotheses; the entry point lives beside the other beam
 * steps in csrc/nm_logits.hip), a companion of nmhip.h with the same conventions: every function returns 0 on success,
 * <0 on error with the text in nm_last_error(); tensor pointers are DEVICE pointers owned by the caller (fp32 / int32);
 * `stream` is a hipStream_t passed as void*; sizes are int64_t element counts.  Arguments are checked before anything
 * is launched.
 *
 * Reference: decoders/beam_search_decoder.py:440-501 (mask, + logprob_sum, length penalty, tf.nn.top_k over [B,k*V]
 * with lower-index-first ties, div/mod, gathers), which puts no bound on the beam size.  nm_beam_topk_step and its
 * two siblings in nmhip.h keep a sorted candidate list of 4 / 8 / 16 entries per thread and stop at k = 16; this entry
 * selects by counting score bins and takes any k up to 64. */
#ifndef NMHIP_BEAM_WIDE_H
#define NMHIP_BEAM_WIDE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* One beam body: inputs and the seven outputs as nm_beam_topk_step_fused (nmhip.h).
 *   score of candidate (j, v) of sentence b: ((x - max) - lse) + logprob_sum, / penalty[len + 1 - finished], the same
 *   four fp32 operations as the narrow kernels; finished rows: lp = 0 at <pad> (word 0), -1e9 elsewhere;
 *   the k best of the k*V scores, exact equality to the lower flat index, outputs ordered by (score descending, flat
 *   index ascending); two runs are bit-equal in every output (integer atomics only, on counts and cursors).
 * Row statistics, in this order of precedence:
 *   rmax_in / rlse_in [B*k] (both or neither): given, e.g. from nm_row_stats, or zeros with log-probabilities for
 *     logits (the ensemble convention); rmax_out / rlse_out are then not written and may be NULL;
 *   stats / tile_w: the tile records of nm_logits_stats_gemm (tile_w 64 or 128, stats 16-byte aligned): max and lse of
 *     every row from the merged records, written to rmax_out / rlse_out;
 *   neither: one pass over the rows computes them into rmax_out / rlse_out.
 * Accepted: 1 <= k <= 64, B >= 1, V >= 1, k*V < 2^31, ldx >= V; any V, any alignment of the rows.
 * workspace: nm_beam_workspace_bytes(B, k, V) bytes (for k <= 16 the narrow kernels' size), 4-byte aligned; it need
 * not be zeroed, the counters in it are reset by the launches themselves.
 * all_finished (or NULL): preset to 1 it ends as int(all out_finished); preset to 0 it stays 0. */
int nm_beam_topk_step_wide(void* stream, const float* logits, int64_t ldx, int64_t B, int64_t k, int64_t V,
                           const float* logprob_sum, const int32_t* lengths, const int32_t* finished,
                           const float* penalty, int end_id, float* out_score, int32_t* out_word,
                           int32_t* out_beam, float* out_logprob_sum, int32_t* out_lengths,
                           int32_t* out_finished, int32_t* out_src_row, void* workspace,
                           int64_t workspace_bytes, int32_t* all_finished, float* rmax_out, float* rlse_out,
                           const float* rmax_in, const float* rlse_in, const float* stats, int64_t tile_w);

#ifdef __cplusplus
}
#endif
#endif
