/* libnmhip -- C ABI of CTC prefix beam search (csrc/nm_ctc_beam.hip), a companion of nmhip_ctc.h with the same
 * conventions: every function returns 0 on success, <0 on error with the text in nm_last_error(); tensor pointers are
 * DEVICE pointers owned by the caller (fp32 / int32); `stream` is a hipStream_t passed as void*; sizes and strides are
 * int64_t element counts.  Arguments are checked before anything is launched.
 *
 * The logits are addressed as x[t*stride_t + b*stride_b + k], t < T frames, b < B sentences, k < K classes with unit
 * class stride; class K-1 is the blank; frame_len[b] <= T frames of sentence b count (nmhip_ctc.h).
 *
 * The search is the recurrence of TensorFlow 1.12's CTCBeamSearchDecoder::Step (tf.nn.ctc_beam_search_decoder) with
 * top_paths = 1, the default scorer and no label selection, on the log-softmax lp of every frame.  A hypothesis is a
 * prefix of non-blank classes with pb / pl, the log mass of its alignments that end in blank / in its last label, and
 * tot = logaddexp(pb, pl); the beam starts with the empty prefix (pb = 0, pl = -inf).  Per frame, from the beam's
 * values `old` before the frame:
 *   survivors   every prefix p of the beam: pb' = old.tot(p) + lp[blank]; pl' = lp[c] + logaddexp(old.pl(p), prev) for a
 *               non-empty p with last label c, where prev comes from p's parent prefix if that is in the beam
 *               (old.pb(parent) if the parent's last label is c too, else old.tot(parent)) and is -inf otherwise; the
 *               empty prefix has pl' = -inf
 *   extensions  p + k for every p of the beam and class k != blank, unless p + k is itself in the beam: pb' = -inf,
 *               pl' = lp[k] + (k == last(p) ? old.pb(p) : old.tot(p)); not a candidate when that is -inf
 *   selection   the beam_size candidates of largest tot' (ties: a survivor first, then the lower beam slot, then the
 *               lower class)
 * After the last frame the prefix of largest tot is written root to leaf; with merge_repeated a label equal to the one
 * emitted before it is dropped (the output only, not the recurrence).  score[b] = that tot, a log-probability.  A
 * sentence with frame_len = 0 emits nothing and scores 0. */
#ifndef NMHIP_CTC_BEAM_H
#define NMHIP_CTC_BEAM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* bytes of the workspace of nm_ctc_beam_search: per frame the row's log-sum-exp, lp[blank] and the
 * min(beam_size + 1, K - 1) best non-blank classes with their lp, per sentence 1 + T * beam_size prefix-tree nodes
 * (parent, label); <0 for sizes the search refuses */
int64_t nm_ctc_beam_workspace_bytes(int64_t B, int64_t T, int64_t K, int64_t beam_size);

/* 1 <= beam_size <= 64, K >= 2.  tokens [B, T] int32 rows hold out_len[b] classes, then end_token; out_len [B] int32;
 * score [B] fp32.  Deterministic: no floating-point atomics, two runs are bit-equal.  Nothing returns to the host. */
int nm_ctc_beam_search(void* stream, const float* logits, int64_t stride_t, int64_t stride_b, int64_t T, int64_t B,
                       int64_t K, const int32_t* frame_len, int64_t beam_size, int merge_repeated, int32_t end_token,
                       int32_t* tokens, int32_t* out_len, float* score, void* workspace, int64_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif
