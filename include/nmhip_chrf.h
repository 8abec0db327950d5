/* libnmhip -- C ABI of the chrF score of sentences (csrc/nm_chrf.hip), a companion of nmhip.h with the same
 * conventions: every function returns 0 on success, <0 on error with the text in nm_last_error(); tensor pointers are
 * DEVICE pointers owned by the caller; `stream` is a hipStream_t passed as void*; sizes and strides are int64_t
 * element counts.  Arguments are checked before anything is launched.
 *
 * The rule is the reference's ChrFEvaluator.score_instance (neuralmonkey/evaluators/chrf.py:35-97) for one reference,
 * stated on the host by SentenceChrF of trainers/self_critical_objective.py:
 *   the sentence of a token column is seq[:e], e the first index that holds end_id or an index outside [0, V), or the
 *   column's length without one (e_1 of nmhip_reward.h): whatever else the decoder emitted is a token;
 *   its text is the tokens' words joined by single spaces; a token whose row carries NM_CHRF_GLUE (a BPE piece "x@@"
 *   under join_subwords) and that has a token of the sentence behind it lends its stem only, and no space follows it;
 *   its characters are the code points of the text without the ignored symbols (the separating space is a character
 *   like any other, and is dropped when " " is ignored: NM_CHRF_SPACE_DROPPED);
 *   with Lh, Lr the numbers of characters of the hypothesis and the reference, for the orders m = 1..n
 *     total_h[m] = max(0, Lh - m + 1), total_r[m] = max(0, Lr - m + 1),
 *     matched[m] = sum over the distinct m-grams of min(count in the hypothesis, count in the reference)
 *     precision  = (sum in order m = 1..n of matched[m] / total_h[m], 1 where total_h[m] == 0) / n, recall with total_r
 *   score = 1 if Lh == Lr == 0, 0 if one of them is 0, 0 if precision == recall == 0, else
 *           (1 + beta^2) (precision recall) / (beta^2 precision + recall)
 *   in double (beta^2 = beta * beta, no contraction), rounded once to float.
 * Integer counts, no atomics: two runs are bit-equal.
 *
 * The character table of a vocabulary of V words (SentenceChrF.table):
 *   rows  int32 [V, 4], 16-byte aligned: (offset, stem_len, whole_len, flags) -- the word's filtered characters are
 *         chars[offset .. offset + whole_len), the first stem_len of them its stem (the text without the trailing
 *         "@@"; stem_len == whole_len for a word without one).  offset + whole_len <= the length of chars is the
 *         caller's to keep: the kernels read where the rows point.  A length is clamped to 0..max_word_chars.
 *   chars uint16: dense ids of the vocabulary's characters, NM_CHRF_SPACE_ID for the space; 0xFFFE and 0xFFFF never
 *         occur (the kernels put them behind the two staged streams). */
#ifndef NMHIP_CHRF_H
#define NMHIP_CHRF_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define NM_CHRF_GLUE 1          /* flags: the word ends in "@@" and pieces are joined */
#define NM_CHRF_SPACE_DROPPED 2 /* flags: " " is an ignored symbol; the same in every row */
#define NM_CHRF_SPACE_ID 0      /* the id of the separating space in chars */
#define NM_CHRF_MAX_ORDER 6

/* the most characters of both staged streams together, by the static bound (T_ref + T_hyp) * (max_word_chars + 1) that
 * sizes a wavefront's dynamic LDS: 16384 characters, 32 788 bytes with the ten fillers.  A training step (T = 50 both
 * sides, words of up to 30 characters) needs 3100 characters = 6220 bytes, so the 160 KiB of a CU hold 26 such
 * wavefronts. */
int64_t nm_chrf_max_chars(void);

/* One score per sentence:
 *   ref [T_ref, B] int32, element (t, b) at ref[t * ref_stride + b]   (time-major, as decoder.train_inputs)
 *   hyp [T_hyp, B] int32, element (t, b) at hyp[t * hyp_stride + b]
 *   reward [B] float; counts [B, 3, 6] int32 (matched, total_h, total_r by order; 0 above n), or null
 * Refused: n outside 1..6, beta not above 0, B < 0, T_ref or T_hyp below 1, V or max_word_chars below 1, a stride
 * below B, a column beyond 2^31 - 1 elements, (T_ref + T_hyp) * (max_word_chars + 1) above nm_chrf_max_chars(), more
 * than 2^25 wavefronts (one per sentence), null pointers (counts excepted), rows not 16-byte aligned.  B == 0 is a
 * no-op. */
int nm_chrf_reward(void* stream, const int32_t* ref, int64_t ref_stride, int64_t T_ref, const int32_t* hyp,
                   int64_t hyp_stride, int64_t T_hyp, int64_t B, int32_t end_id, const int32_t* rows,
                   const uint16_t* chars, int64_t V, int64_t max_word_chars, int n, double beta, float* reward,
                   int32_t* counts);

/* The utilities of minimum Bayes risk decoding over the samples tok [T, B, n_samples] of nmhip_mbr.h (element
 * (t, b, j) at tok[t * t_stride + b * n_samples + j]):  U [B, n_samples, n_samples] float,
 * U[b, i, j] = chrF(reference = sample j, hypothesis = sample i).  matched is symmetric: a pair i < j is expanded and
 * matched once and finished in both directions (precision and recall swap); U[b, i, i] = 1 is written without
 * matching anything.
 * Refused: as above, and n_samples outside 1..64, t_stride < B * n_samples, T * t_stride or B * n_samples^2 beyond
 * 2^31 - 1, 2 * T * (max_word_chars + 1) above nm_chrf_max_chars(), more than 2^25 wavefronts (one per pair i < j). */
int nm_chrf_pairwise(void* stream, const int32_t* tok, int64_t t_stride, int64_t T, int64_t B, int64_t n_samples,
                     int32_t end_id, const int32_t* rows, const uint16_t* chars, int64_t V, int64_t max_word_chars,
                     int n, double beta, float* U);

#ifdef __cplusplus
}
#endif
#endif
