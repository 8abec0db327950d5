/* libnmhip -- C ABI of supervised attention (csrc/nm_align.hip), a companion of nmhip.h with the same conventions: every
 * function returns 0 on success, <0 on error with the text in nm_last_error(); tensor pointers are DEVICE pointers owned
 * by the caller (fp32); `stream` is a hipStream_t passed as void*; sizes and strides are int64_t element counts.
 * Arguments are checked before anything is launched.
 *
 * Reference: neuralmonkey/decoders/word_alignment_decoder.py.  w are the attention WEIGHTS the teacher-forced (or the
 * runtime) loop recorded (attention/feed_forward.py:189), time-major and dense: w[(t*B + b)*S + s].  The reference takes
 * its softmax over them, padded source positions (weight 0) included; so do these kernels. */
#ifndef NMHIP_ALIGN_H
#define NMHIP_ALIGN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* word_alignment_decoder.py:100-108 in one launch, one wavefront per (t, b) row.  The label of (t, b, s) is read IN PLACE
 * from the batch-major fed array at target[b*tgt_stride_b + t*tgt_stride_t + s]: rows t >= T and columns s >= S of that
 * array are never read.  With lse = log sum_s exp(w[t,b,s]):
 *   loss_rows[t,b] = pad[t,b] * sum_s label_s * (lse - w[t,b,s])                                    [T, B]
 *   dw[t,b,s]      = scale * pad[t,b] * (softmax(w[t,b,:])_s - label_s)   [T, B, S] or NULL: no gradient
 * -- the gradient TensorFlow 1.12 registers for softmax_cross_entropy_with_logits (the incoming gradient times the op's
 * second output), whatever the labels sum to: an all-zero label row has loss 0 and gradient scale * pad * softmax(w).
 * accumulate != 0 adds onto what dw holds, 0 overwrites.  scale: one DEVICE float (NULL = 1).  A row with pad == 0 gets
 * an exact 0 loss and exact 0 gradient and its labels are not read.  No atomics: two runs are bit-equal.
 * Refused: null w, target, pad or loss_rows; T, B or S < 0; S < 1 with rows present; tgt_stride_t < S;
 * tgt_stride_b < T * tgt_stride_t; T*B beyond 2^31 - 1; dw aliasing w.  T*B == 0 is a no-op. */
int nm_align_xent(void* stream, const float* w, int64_t T, int64_t B, int64_t S, const float* target,
                  int64_t tgt_stride_b, int64_t tgt_stride_t, const float* pad, const float* scale, float* loss_rows,
                  float* dw, int accumulate);

/* word_alignment_decoder.py:91-97: out[b, t, :] = softmax(w[t, b, :]), batch-major [B, T, S].  Refused: null pointers,
 * bad sizes as above, out aliasing w.  T*B == 0 is a no-op. */
int nm_align_softmax(void* stream, const float* w, int64_t T, int64_t B, int64_t S, float* out);

#ifdef __cplusplus
}
#endif
#endif
