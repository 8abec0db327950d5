/* libnmhip -- C ABI of REINFORCE training with sentence-level feedback (csrc/nm_rl.hip), a companion of nmhip.h with
 * the same conventions: every function returns 0 on success, <0 on error with the text in nm_last_error(); tensor
 * pointers are DEVICE pointers owned by the caller (fp32 / int32) unless said otherwise; `stream` is a hipStream_t
 * passed as void*; sizes and strides are int64_t element counts.  Arguments are checked before anything is launched.
 *
 * Reference: neuralmonkey/trainers/rl_trainer.py, where the reward is an Evaluator object called once per sentence and
 * per sample behind tf.py_func (sample_size x B joins and splits of Python strings and a device-to-host read-back per
 * sample), and neuralmonkey/evaluators/{bleu,gleu}.py. */
#ifndef NMHIP_RL_H
#define NMHIP_RL_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* the largest T_ref + T_hyp nm_eval_sentence_score takes: both token columns of a sentence are staged in the LDS of
 * the one wavefront that scores it (4 bytes per token, 8192 tokens = 32 KiB) */
int64_t nm_eval_sentence_score_max_tokens(void);

/* rl_trainer.py:83-115 (_score_with_reward_function) with evaluators/gleu.py:47-110 (kind 1) or evaluators/bleu.py:
 * 98-133,196-236 (kind 0) as the reward, on token indices, one score per sentence -- valid where equal words are equal
 * indices (no word of the vocabulary ends with "@@", is empty or holds a space: the join of rl_trainer.py:110-111 is
 * then the identity).
 *   ref [T_ref, B] int32, element (t, b) at ref[t * ref_stride + b]   (time-major, as decoder.train_inputs)
 *   hyp [T_hyp, B] int32, element (t, b) at hyp[t * hyp_stride + b]   (the sampled symbols); T_ref != T_hyp is fine
 *   out [B] float
 * Words: a column is cut at its first end_id OR pad_id (rl_trainer.py:99-108); token ids are >= 0.  A column that is
 * empty then is ONE word, the empty string ("".split(" ") == [""]), equal only to the word of another empty column.
 * Counts, for n = 1 .. order (all integers): gen_n = max(0, |hyp| - n + 1), tgt_n = max(0, |ref| - n + 1) and tp_n = the
 * number of reference windows of n words that equal SOME hypothesis window -- the evaluators add the reference's count
 * over the DISTINCT hypothesis n-grams (bleu.py:122-124, gleu.py:80-82), which is not a clipped count.
 *   GLEU: min(sum tp / sum gen, sum tp / sum tgt)
 *   BLEU: 100 * exp(sum_n (1 / order) * log prec_n + min(1 - |ref| / |hyp|, 0)) with prec_n = tp_n / gen_n, 1 where
 *         gen_n == 0, and where it is 0 the smoothing of mteval-v13a that runs across the orders: smooth *= 2,
 *         prec_n = 1 / (smooth * gen_n)  (bleu.py:212-236)
 * The final arithmetic is double, rounded once to float.  One wavefront per sentence and no atomics: two runs are
 * bit-equal.  Refused: kind outside {0, 1}, order outside 1..4, B < 0, T_ref < 1, T_hyp < 1,
 * T_ref + T_hyp > nm_eval_sentence_score_max_tokens(), a stride below B, a column beyond 2^31 - 1 elements,
 * end_id == pad_id or a negative one, null pointers.  B == 0 is a no-op. */
int nm_eval_sentence_score(void* stream, int kind, int order, const int32_t* ref, int64_t ref_stride, int64_t T_ref,
                           const int32_t* hyp, int64_t hyp_stride, int64_t T_hyp, int64_t B, int32_t end_id,
                           int32_t pad_id, float* out);

/* the largest S (sample_size) nm_reinforce_sample_weights takes: the loop lengths travel as a launch argument */
int64_t nm_reinforce_sample_weights_max_samples(void);

/* rl_trainer.py:149-185: the running-average baseline, the normalisation over the sample space and the loss, as the
 * operands of nm_xent (nmhip.h) over each sample's logits with the sampled symbols as targets -- one launch, one
 * workgroup, nothing read back.
 *   rewards       [S, B] float
 *   sent_logprobs [S, B] float: minus the sum of the nll over ALL steps of the sample's loop (:135-140).  May be null
 *                 without `normalize`; the loss is not written then (it is the sum of nm_xent's loss rows).
 *   steps         HOST array of S loop lengths, 1 <= steps[s] <= T (the host has read them to end the loops)
 *   reward_counter, reward_sum   [1] float each, the baseline's state, updated in place BEFORE use (:155-163):
 *                 counter += B * S, sum += sum(rewards), baseline = sum / max(counter, 1) -- float32 throughout (the
 *                 reference's reduce_sum accumulates in float32 too), the rewards added up as eight interleaved partial
 *                 sums (element i to sum i % 8) combined as ((0+1)+(2+3))+((4+5)+(6+7)), then the S * B % 8 last ones in
 *                 order; fewer than eight in order.  ONE lane adds them up while the workgroup waits: S * B / 8 dependent
 *                 additions per chain -- a microsecond at a training step's S * B of a few hundred, but S = 64 with
 *                 B in the thousands is 10^5 loads on one lane: of the order of a millisecond.  Read and written with
 *                 `subtract_baseline` only; may be null without it (baseline = 0).
 * With a_s = -(rewards[s, b] - baseline):
 *   without normalize   loss = 1/B sum_b sum_s a_s * sent_logprobs[s, b];   d loss / d sent_logprobs[s, b] = a_s / B
 *   with normalize      p = softmax_s(alpha * sent_logprobs[:, b]) (:170-173), loss = 1/B sum_b sum_s a_s p_s,
 *                       d loss / d sent_logprobs[s, b] = alpha p_s (a_s - sum_s' a_s' p_s') / B
 *   weights[(s * T + t) * B + b] = -d loss / d sent_logprobs[s, b] for t < steps[s], 0 behind it     [S, T, B] float
 *   grad_scale[0] = weight     (the objective's weight; a caller that divided the logits by a temperature folds 1 /
 *                               temperature in)
 *   loss[0], baseline[0]       [1] float each; loss may be null
 * The weights and the loss are computed in double from the float32 inputs and the float32 baseline, summed in a fixed
 * order, and rounded once: two runs are bit-equal.  Refused: S outside
 * 1..nm_reinforce_sample_weights_max_samples(), T < 1, B < 1, S * T * B beyond 2^31 - 1, a loop length outside 1..T,
 * normalize without sent_logprobs, subtract_baseline without its state, null pointers. */
int nm_reinforce_sample_weights(void* stream, const float* rewards, const float* sent_logprobs, const int32_t* steps,
                                int64_t S, int64_t T, int64_t B, int subtract_baseline, int normalize, float alpha,
                                float weight, float* reward_counter, float* reward_sum, float* weights,
                                float* grad_scale, float* loss, float* baseline);

#ifdef __cplusplus
}
#endif
#endif
