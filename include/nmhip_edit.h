/* libnmhip -- C ABI of the edit-distance scores of sentences (csrc/nm_edit.hip), a companion of nmhip.h with the same
 * conventions: every function returns 0 on success, <0 on error with the text in nm_last_error(); tensor pointers are
 * DEVICE pointers owned by the caller (fp32 / int32); `stream` is a hipStream_t passed as void*; sizes and strides are
 * int64_t element counts.  Arguments are checked before anything is launched.
 *
 * The reference has no such score; the rule is this project's own, stated on the host by
 * sentence_edit_accuracy / sentence_neg_wer of trainers/self_critical_objective.py:
 *   the sentence of a token column is seq[:e], e the first index that holds end_id, or the column's length without
 *   one (e_1 of nmhip_reward.h): whatever else the decoder emitted, <pad> included, is a token;
 *   d is the Levenshtein distance of the two sentences over token indices (insertion, deletion, substitution cost 1);
 *   with lr, lh the lengths of the reference's and the hypothesis' sentence
 *     kind 0, edit accuracy:  1 - d / max(lr, lh), and 1 when both are empty   (symmetric, in [0, 1])
 *     kind 1, negative WER:   -d / max(lr, 1)
 *   computed in double from the integers and rounded once to float.
 * Integer arithmetic, no atomics: two runs are bit-equal. */
#ifndef NMHIP_EDIT_H
#define NMHIP_EDIT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* the longest token column either kernel takes: a lane of the wavefront that owns a pair keeps 16 columns of the
 * dynamic-programming table in registers, 64 lanes x 16 = 1024 */
int64_t nm_edit_max_tokens(void);

/* One score per sentence:
 *   ref [T_ref, B] int32, element (t, b) at ref[t * ref_stride + b]   (time-major, as decoder.train_inputs)
 *   hyp [T_hyp, B] int32, element (t, b) at hyp[t * hyp_stride + b]   T_ref != T_hyp is fine
 *   reward [B] float; dist [B] int32, the distances d themselves, or null
 * Refused: kind outside {0, 1}, B < 0, T_ref or T_hyp outside 1..nm_edit_max_tokens(), a stride below B, a column
 * beyond 2^31 - 1 elements, more than 2^25 wavefronts (of 4, 2 or 1 sentences at T_hyp <= 16, <= 32, above), null
 * pointers (dist excepted).  B == 0 is a no-op. */
int nm_edit_reward(void* stream, int kind, const int32_t* ref, int64_t ref_stride, int64_t T_ref, const int32_t* hyp,
                   int64_t hyp_stride, int64_t T_hyp, int64_t B, int32_t end_id, float* reward, int32_t* dist);

/* The utilities of minimum Bayes risk decoding over the samples tok [T, B, n] of nmhip_mbr.h (element (t, b, j) at
 * tok[t * t_stride + b * n + j]):  U [B, n, n] float, U[b, i, j] = score(reference = sample j, hypothesis = sample i).
 * d is symmetric: a pair i < j is computed once and finished in both directions; U[b, i, i] (1 for kind 0, 0 for
 * kind 1) is written without a distance being computed.
 * Refused: kind outside {0, 1}, n outside 1..64, T outside 1..nm_edit_max_tokens(), B < 0, t_stride < B * n,
 * T * t_stride or B * n * n beyond 2^31 - 1, B n (n - 1) / 2 pairs in more than 2^25 wavefronts (of 4, 2 or 1 pairs
 * at T <= 16, <= 32, above), null pointers.  B == 0 is a no-op. */
int nm_edit_pairwise(void* stream, int kind, const int32_t* tok, int64_t t_stride, int64_t T, int64_t B, int64_t n,
                     int32_t end_id, float* U);

#ifdef __cplusplus
}
#endif
#endif
