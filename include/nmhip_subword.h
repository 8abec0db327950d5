/* libnmhip -- C ABI of the REINFORCE reward over a vocabulary of subword pieces (csrc/nm_subword.hip), a companion of
 * nmhip_rl.h with the same conventions: every function returns 0 on success, <0 on error with the text in
 * nm_last_error(); tensor pointers are DEVICE pointers owned by the caller (fp32 / int32); `stream` is a hipStream_t
 * passed as void*; sizes and strides are int64_t element counts.  Arguments are checked before anything is launched.
 *
 * Reference: neuralmonkey/trainers/rl_trainer.py:83-115 (_score_with_reward_function), whose join of BPE pieces
 * (:110-111, " ".join(tokens).replace("@@ ", "").split(" ")) makes two different piece sequences one word, and
 * neuralmonkey/evaluators/{bleu,gleu}.py. */
#ifndef NMHIP_SUBWORD_H
#define NMHIP_SUBWORD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* the largest T_ref + T_hyp nm_eval_joined_sentence_score takes (8192): the one wavefront that scores a sentence keeps
 * 12 bytes per word of both columns and 4 bytes per token of the longer one in LDS, 128 KiB of the CU's 160 KiB */
int64_t nm_eval_joined_sentence_score_max_tokens(void);

/* rl_trainer.py:83-115 with evaluators/gleu.py:47-110 (kind 1) or evaluators/bleu.py:98-133,196-236 (kind 0) as the
 * reward, on the indices of PIECES, one score per sentence -- for a vocabulary in which no word is empty and none holds
 * a space.
 *   ref [T_ref, B] int32, element (t, b) at ref[t * ref_stride + b]   (time-major, as decoder.train_inputs)
 *   hyp [T_hyp, B] int32, element (t, b) at hyp[t * hyp_stride + b]   (the sampled symbols); T_ref != T_hyp is fine
 *   table [table_rows, 12] int32, one row per vocabulary entry, table_rows >= V, built ONCE per vocabulary on the host:
 *         [0..4]  of the STEM (the text without a trailing "@@"; the whole text where there is none): hash modulo M1,
 *                 hash modulo M2, P1^len modulo M1, P2^len modulo M2, len (UTF-8 bytes)
 *         [5..9]  the same five of the WHOLE text
 *         [10]    bit 0: the text ends with "@@" (a continuation piece); bit 1: the text is "</s>" or "<pad>" (the cut
 *                 is decided by this flag, as the reference decides it by string -- a vocabulary may repeat a word)
 *         [11]    0
 *         with H(s) = sum_i (byte_i + 1) * P^(len - 1 - i) modulo M, (M1, P1) = (2^31 - 1, 1103515245) and
 *         (M2, P2) = (2^31 - 19, 1664525), so that H(s + t) = H(s) * P^len(t) + H(t): a word's hash is composed from its
 *         pieces' without touching a character
 *   out [B] float
 * The cut: a column ends before its first token whose flag has bit 1 set.  A token id outside [0, V) is treated as such
 * a token too (it CUTS the column; the table is never read outside its V rows).
 * The join (:110-111): a kept token that is a continuation piece and not the last kept token contributes its stem as a
 * prefix of the next word; every other kept token ends a word with its whole text -- so a last kept token that ends with
 * "@@" keeps it, and a token that is just "@@" contributes the empty prefix.  An empty column is ONE word, the empty
 * string; no joined word of a non-empty column is empty.  Lengths are counted in joined words, not in pieces.
 * Word identity: two words are taken for equal when their (length in bytes, hash modulo M1, hash modulo M2) are equal.
 * THIS IS THE ONE PLACE WHERE THE DEVICE ROUTE IS NOT EXACT BY CONSTRUCTION: equal words always compare equal, and two
 * DIFFERENT words of one length L compare equal when both polynomial hashes collide -- for bases drawn at random at most
 * ((L - 1) / 2^31)^2 per comparison (about 8e-17 for words of 20 bytes, 62 bits of hash); the bases are fixed constants,
 * so this is the figure for text that was not built against them.  Words of different lengths never compare equal.  No
 * pass over the characters verifies a match.
 * Counts, for n = 1 .. order (all integers), exactly those of nm_eval_sentence_score (nmhip_rl.h): gen_n, tgt_n and
 * tp_n = the number of reference windows of n words that equal SOME hypothesis window -- not a clipped count
 * (bleu.py:122-124, gleu.py:80-82); GLEU = min(sum tp / sum gen, sum tp / sum tgt), BLEU with the smoothing of
 * mteval-v13a across the orders and the brevity term, times 100 (bleu.py:212-236).  The final arithmetic is double,
 * rounded once to float.  One wavefront per sentence and no atomics: two runs are bit-equal.
 * Refused: kind outside {0, 1}, order outside 1..4, B < 0, T_ref < 1, T_hyp < 1,
 * T_ref + T_hyp > nm_eval_joined_sentence_score_max_tokens(), a stride below B, a column beyond 2^31 - 1 elements,
 * V < 1 or beyond 2^31 - 1, table_rows < V, null pointers.  B == 0 is a no-op. */
int nm_eval_joined_sentence_score(void* stream, int kind, int order, const int32_t* ref, int64_t ref_stride,
                                  int64_t T_ref, const int32_t* hyp, int64_t hyp_stride, int64_t T_hyp, int64_t B,
                                  const int32_t* table, int64_t table_rows, int64_t V, float* out);

#ifdef __cplusplus
}
#endif
#endif
