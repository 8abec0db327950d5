/* libnmhip -- C ABI of minimum Bayes risk decoding over the samples of a sentence (csrc/nm_mbr.hip), a companion of
 * nmhip.h with the same conventions: every function returns 0 on success, <0 on error with the text in
 * nm_last_error(); tensor pointers are DEVICE pointers owned by the caller (fp32 / int32); `stream` is a hipStream_t
 * passed as void*; sizes and strides are int64_t element counts.  Arguments are checked before anything is launched.
 *
 * The reference has no such decoder; the rule is this project's own.  The utilities are the
 * reference's sentence_bleu / sentence_gleu (neuralmonkey/trainers/self_critical_objective.py:124-231) exactly as
 * nmhip_reward.h states them.
 *
 * The samples: tok [T, B, n] int32, sample j of sentence b is the column (b, j), element (t, b, j) at
 * tok[t * t_stride + b * n + j] -- what SamplingDecoder writes: </s> where a sample ended, <pad> behind it. */
#ifndef NMHIP_MBR_H
#define NMHIP_MBR_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* U [B, n, n] float: U[b, i, j] = utility(reference = sample j, hypothesis = sample i) of sentence b; kind 0 is
 * sentence_bleu, kind 1 sentence_gleu, with the ends e_n, the clipped counts and BLEU's + 1 for n > 1 of
 * nm_sentence_reward (nmhip_reward.h).  The counts are integers, the final arithmetic is double, rounded once to float.
 * The clipped count of a pair does not depend on which of the two is the hypothesis, so one wavefront scores an
 * unordered pair i <= j in one matching pass and writes both U[b, i, j] and U[b, j, i]; GLEU is therefore symmetric
 * bit for bit.  No atomics: two runs are bit-equal.
 * Refused: kind outside {0, 1}, n outside 1..64, T < 1, B < 0, 2 * T > nm_sentence_reward_max_tokens(),
 * t_stride < B * n, T * t_stride or B * n * n beyond 2^31 - 1, end_id < 0, null pointers.  B == 0 is a no-op. */
int nm_mbr_pairwise(void* stream, int kind, const int32_t* tok, int64_t t_stride, int64_t T, int64_t B, int64_t n,
                    int32_t end_id, float* U);

/* The choice, from utilities U [B, n, n] of any origin (nm_mbr_pairwise's, or a host function's):
 *   S[b, i]        = sum over j = 0 .. n - 1, in that order, of (double) U[b, i, j]     (i == j included)
 *   expected[b, i] = (float)(S[b, i] / n)                                               [B, n] float
 *   best[b]        = argmax over i of S[b, i] on the double sums; ties go to the lowest i, a NaN sorts behind
 *                    everything, 0 if every sum is NaN                                  [B] int32
 *   chosen[t, b]   = tok[t * t_stride + b * n + best[b]], t < T                         [T, B] int32, contiguous
 * One wavefront per sentence, no atomics: two runs are bit-equal.
 * Refused: n outside 1..64, T < 1, B < 0, t_stride < B * n, T * t_stride or B * n * n beyond 2^31 - 1, null
 * pointers.  B == 0 is a no-op. */
int nm_mbr_select(void* stream, const float* U, const int32_t* tok, int64_t t_stride, int64_t T, int64_t B, int64_t n,
                  float* expected, int32_t* best, int32_t* chosen);

#ifdef __cplusplus
}
#endif
#endif
