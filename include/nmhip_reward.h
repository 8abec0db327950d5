/* libnmhip -- C ABI of the sentence-level rewards of self-critical training (csrc/nm_reward.hip), a companion of
 * nmhip.h with the same conventions: every function returns 0 on success, <0 on error with the text in
 * nm_last_error(); tensor pointers are DEVICE pointers owned by the caller (fp32 / int32); `stream` is a hipStream_t
 * passed as void*; sizes and strides are int64_t element counts.  Arguments are checked before anything is launched.
 *
 * Reference: neuralmonkey/trainers/self_critical_objective.py, where the rewards are Python functions behind
 * tf.py_func (two device-to-host read-backs per step, four Counter loops per sentence and per decoding). */
#ifndef NMHIP_REWARD_H
#define NMHIP_REWARD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* the largest T_ref + T_hyp nm_sentence_reward takes: both token columns of a sentence are staged in the LDS of the
 * one wavefront that scores it (4 bytes per token, 8192 tokens = 32 KiB) */
int64_t nm_sentence_reward_max_tokens(void);

/* self_critical_objective.py:124-162 (sentence_bleu, kind 0) and :165-200 (sentence_gleu, kind 1) with their helpers
 * :203-225 (_count_matching_n_grams) and :228-231 (_get_n_grams), on token indices, one score per sentence.
 *   ref [T_ref, B] int32, element (t, b) at ref[t * ref_stride + b]   (time-major, as decoder.train_inputs)
 *   hyp [T_hyp, B] int32, element (t, b) at hyp[t * hyp_stride + b]   (the argmax of the logits); T_ref != T_hyp is fine
 *   out [B] float
 * For the orders n = 1..4 the n-grams of a sequence s of length T are its windows s[i .. i+n-1] with i + n - 1 < e_n,
 * where e_n is the first index >= n - 1 that holds end_id, or T without one (an end token below index n - 1 ends
 * nothing); total_n = max(0, e_n - n + 1).  matched_n is the clipped count: the hypothesis window at i matches iff
 * fewer equal hypothesis windows start before i than there are equal reference windows.
 *   BLEU: matched_n and the hypothesis' total_n grow by 1 for n > 1; 0 if the hypothesis has no unigram, else
 *         (prod matched / prod total)^(1/4) * min(1, exp(1 - e_1(ref) / total_1(hyp)))
 *   GLEU: min(sum matched / sum total(hyp), sum matched / sum total(ref)); 0 where either sum of totals is 0 (the
 *         reference fails its own assertion there)
 * The counts are integers, the final arithmetic is double, rounded once to float.  One wavefront per sentence and no
 * atomics: two runs are bit-equal.  Refused: kind outside {0, 1}, B < 0, T_ref < 1, T_hyp < 1,
 * T_ref + T_hyp > nm_sentence_reward_max_tokens(), a stride below B, a column beyond 2^31 - 1 elements, null pointers.
 * B == 0 is a no-op. */
int nm_sentence_reward(void* stream, int kind, const int32_t* ref, int64_t ref_stride, int64_t T_ref,
                       const int32_t* hyp, int64_t hyp_stride, int64_t T_hyp, int64_t B, int32_t end_id, float* out);

/* self_critical_objective.py:75-85 and :113-120 (reinforce_score), as the operands of nm_xent (nmhip.h) over the
 * runtime logits with the decoded symbols as targets -- nothing is read back to the host:
 *   weights[t * B + b] = -(reward[b] - baseline[b]) * mask[t * B + b]      [T, B] float, the row weights
 *   grad_scale[0]      = weight / sum(mask)                                the device scalar of the gradient
 *   inv_count[0]       = 1 / sum(mask)                                     ... and of the reported loss
 * mask [T, B] int32 is the runtime mask (contiguous); reward, baseline [B] float.  With sum(mask) == 0 both scalars
 * are 0 (no gradient; the reference divides by zero).  One workgroup, integer count: deterministic.  Refused: T < 1,
 * B < 1, T * B beyond 2^31 - 1, null pointers. */
int nm_reinforce_weights(void* stream, const float* reward, const float* baseline, const int32_t* mask, int64_t T,
                         int64_t B, float weight, float* weights, float* grad_scale, float* inv_count);

#ifdef __cplusplus
}
#endif
#endif
