/* libnmhip -- C ABI of the CTC head (csrc/nm_ctc.hip), a companion of nmhip.h with the same conventions: every
 * function returns 0 on success, <0 on error with the text in nm_last_error(); tensor pointers are DEVICE pointers
 * owned by the caller (fp32 / int32); `stream` is a hipStream_t passed as void*; sizes and strides are int64_t
 * element counts.  Arguments are checked before anything is launched.
 *
 * Reference: neuralmonkey/decoders/ctc_decoder.py.  The logits are addressed as x[t*stride_t + b*stride_b + k],
 * t < T frames, b < B sentences, k < K classes with unit class stride -- the time-major [T, B, K] tensor of
 * ctc_decoder.py:140 without the transpose; class K-1 is the blank (tf.nn.ctc_loss: num_classes - 1).
 * labels [B, Lmax] int32 rows hold label_len[b] classes in [0, K-1) (pad positions removed, repeats collapsed by the
 * caller when preprocess_collapse_repeated is set); frame_len[b] <= T frames of sentence b count. */
#ifndef NMHIP_CTC_H
#define NMHIP_CTC_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* bytes of the workspace the three calls below share for sentences of at most Lmax labels: row log-sum-exps and
 * argmax classes [B*T], alpha and beta [B, T, 2 Lmax + 1], per sentence log Z / validity / same-class label links */
int64_t nm_ctc_workspace_bytes(int64_t B, int64_t T, int64_t Lmax);

/* model/stateful.py:55-62 (TemporalStateful.lengths = reduce_sum(temporal_mask, 1) as int32): lengths[b] = the sum
 * of the 0/1 float row mask[b*ld .. +T) */
int nm_ctc_mask_lengths(void* stream, const float* mask, int64_t ld, int64_t B, int64_t T, int32_t* lengths);

/* ctc_decoder.py:100-108, tf.nn.ctc_loss(ignore_longer_outputs_than_inputs=True, ctc_merge_repeated=merge_repeated)
 * + tf.reduce_sum: loss[b] = -log sum over the alignments of sentence b of the product of their softmax emissions,
 * loss_sum[0] = the sum over the batch (added in a fixed order).  merge_repeated != 0: a label state loops on
 * itself and equal neighbours need a blank between them; 0: label states have no self-loop and the skip over a blank
 * is allowed between equal labels.  A sentence without an alignment (zero frames, or more labels -- plus blanks
 * between repeats when merging -- than frames) has loss 0 and, in nm_ctc_loss_bwd, gradient 0; an empty label
 * sequence is the all-blank path.  A label outside [0, K-1) gives that sentence loss NaN and gradient 0.  The
 * workspace keeps what nm_ctc_loss_bwd reads. */
int nm_ctc_loss_fwd(void* stream, const float* logits, int64_t stride_t, int64_t stride_b, int64_t T, int64_t B,
                    int64_t K, const int32_t* labels, int64_t Lmax, const int32_t* label_len, const int32_t* frame_len,
                    int merge_repeated, float* loss, float* loss_sum, void* workspace, int64_t workspace_bytes);

/* tf.gradients of the above w.r.t. the logits (generic_trainer.py:96-100), after nm_ctc_loss_fwd on the same
 * operands and workspace: dlogits[t, b, k] = scale[0] * (softmax(logits[t, b])[k] - occupancy[t, b, k]), where
 * occupancy is the posterior mass of the states of the blank-interleaved labels that carry class k; exact zeros for
 * t >= frame_len[b] and for sentences without an alignment.  scale: one DEVICE float (NULL = 1).  dlogits has strides
 * of its own and may be the logits themselves (in place).  Deterministic: no floating-point atomics. */
int nm_ctc_loss_bwd(void* stream, const float* logits, int64_t stride_t, int64_t stride_b, int64_t T, int64_t B,
                    int64_t K, const int32_t* labels, int64_t Lmax, const int32_t* label_len, const int32_t* frame_len,
                    const float* scale, float* dlogits, int64_t dstride_t, int64_t dstride_b, const void* workspace,
                    int64_t workspace_bytes);

/* ctc_decoder.py:76-89, tf.nn.ctc_greedy_decoder(merge_repeated) + sparse_tensor_to_dense(default END): per frame
 * t < frame_len[b] the argmax class (ties: the lowest), emitted unless it is the blank or -- with merge_repeated --
 * equals the previous frame's class; tokens [B, T] int32 rows hold out_len[b] emitted classes, then end_token.
 * Workspace: nm_ctc_workspace_bytes(B, T, 0) bytes suffice. */
int nm_ctc_greedy(void* stream, const float* logits, int64_t stride_t, int64_t stride_b, int64_t T, int64_t B, int64_t K,
                  const int32_t* frame_len, int merge_repeated, int32_t end_token, int32_t* tokens, int32_t* out_len,
                  void* workspace, int64_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif
