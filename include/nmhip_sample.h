/* libnmhip -- C ABI of the truncated sampling step (temperature, top-k and nucleus sampling with a log-probability per
 * draw; csrc/nm_sample.hip), a companion of nmhip.h with the same conventions: every function returns 0 on success,
 * <0 on error with the text in nm_last_error(); tensor pointers are DEVICE pointers owned by the caller (fp32 / int32);
 * `stream` is a hipStream_t passed as void*; sizes are int64_t element counts.  Arguments are checked before anything
 * is launched.
 *
 * The reference has no such decoding mode (its only stochastic loop is tf.multinomial over the whole vocabulary,
 * decoders/autoregressive.py:470-473, which nm_gumbel_argmax of nmhip.h mirrors); the rule is this project's own
 * (DESIGN section 4.9b). */
#ifndef NMHIP_SAMPLE_H
#define NMHIP_SAMPLE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* One sampling step over `rows` rows of `V` logits (row stride ldx).  For an unfinished row r:
 *   z[c] = x[r,c] * inv_temperature (one fp32 multiply); the entries are ordered by (z descending, column ascending);
 *   the kept set S is a prefix of that order: the first top_k entries (top_k == 0 or >= V: all of them), cut, when
 *   top_p < 1, to the shortest prefix whose softmax mass is >= top_p * (mass of the top-k prefix); S is never empty;
 *   symbol = argmax over S of z[c] - logf(-logf(u[r,c])), u the hash of nm_gumbel_argmax with the salt
 *   *salt_base + salt_step, ties to the lower column (with top_k == 0, top_p == 1 and inv_temperature == 1 the symbol
 *   is bit-equal to nm_gumbel_argmax's);
 *   out_logprob = z[symbol] - log(sum over S of exp(z)), out_kept = |S|.
 * A finished row (finished[r] != 0): symbol 0 (<pad>), logprob 0, kept 0.
 * Loop state: out_finished = finished | (symbol == end_id), out_lengths = lengths + !finished,
 *   out_logprob_sum = logprob_sum + out_logprob.  The outputs may alias their inputs.
 * all_finished (or NULL): preset to 1 it ends as int(all out_finished); preset to 0 it stays 0.
 * salt_base: DEVICE pointer to one uint32 (a captured graph draws afresh when the word is rewritten between replays).
 * A row of NaN or -inf still yields a symbol in [0, V).  Two runs are bit-equal in every output: the masses that
 * decide the nucleus boundary are sums of fixed-point terms, round(exp(z - max) * 2^31), in 64-bit integers.
 * Accepted: rows >= 0, 1 <= V < 2^30, ldx >= V, any alignment of the rows, top_k >= 0, 0 < top_p <= 1,
 * inv_temperature > 0 and finite.  workspace: not needed, may be NULL (workspace_bytes >= 0). */
int nm_sample_step(void* stream, const float* logits, int64_t ldx, int64_t rows, int64_t V, float inv_temperature,
                   int64_t top_k, float top_p, const uint32_t* salt_base, uint32_t salt_step, int end_id,
                   const int32_t* finished, const float* logprob_sum, const int32_t* lengths, int32_t* out_symbol,
                   float* out_logprob, int32_t* out_kept, int32_t* out_finished, float* out_logprob_sum,
                   int32_t* out_lengths, int32_t* all_finished, void* workspace, int64_t workspace_bytes);

/* The longest row that nm_sample_step keeps resident in LDS; longer rows are re-read from memory by every pass. */
int64_t nm_sample_lds_max_columns(void);

#ifdef __cplusplus
}
#endif
#endif
