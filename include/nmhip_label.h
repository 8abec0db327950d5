/* libnmhip -- C ABI of the sequence-labelling head (csrc/nm_label.hip), a companion of nmhip.h with the same
 * conventions: every function returns 0 on success, <0 on error with the text in nm_last_error(); tensor pointers are
 * DEVICE pointers owned by the caller (fp32 / int32); `stream` is a hipStream_t passed as void*; sizes and leading
 * dimensions are int64_t element counts.  Arguments are checked before anything is launched.
 *
 * Reference: neuralmonkey/decoders/sequence_labeler.py.  logits are rows x[r*ld + k], r < rows = B*T, k < K classes
 * with unit class stride. */
#ifndef NMHIP_LABEL_H
#define NMHIP_LABEL_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* the largest K nm_label_rows takes (one wavefront holds a row in at most 16 registers per lane) */
int64_t nm_label_rows_max_classes(void);

/* sequence_labeler.py:114-129 in one pass over the rows.  With m the row maximum, lse = log sum exp(x - m),
 * t = targets[r] and w = (t != pad_id) -- sentence_mask of the TARGETS, not the encoder's mask:
 *   loss_rows[r]  = w ? (m + lse - x[t]) : 0 (an exact zero)            [rows] or NULL
 *   logprobs[r,k] = x[k] - m - lse   (tf.nn.log_softmax)                [rows, K] with leading dimension ldp, or NULL;
 *                                                                       must not overlap the logits
 *   argmax[r]     = tf.argmax: the first maximum wins                   [rows] or NULL
 *   labels[r]     = row_mask[r] != 0 ? argmax : masked_class            [rows] or NULL (needs row_mask [rows])
 *   write_grad:     x[k] <- scale * w * (softmax(x)[k] - [k == t]) IN PLACE; rows with w = 0 get exact zeros
 * targets NULL: inference -- no loss, no gradient.  grad_scale: one DEVICE float (NULL = 1).  A target outside [0, K)
 * that is not pad_id gives that row loss NaN and gradient 0.  A row may hold -inf classes.  The row is read once and
 * written at most once; two runs are bit-equal (no floating-point atomics).  Refused: K < 1,
 * K > nm_label_rows_max_classes(), ld < K, ldp < K with logprobs, write_grad without targets, logprobs overlapping the
 * logits, labels without row_mask.  rows == 0 is a no-op. */
int nm_label_rows(void* stream, float* logits, int64_t ld, int64_t rows, int64_t K, const int32_t* targets,
                  int32_t pad_id, const float* grad_scale, int write_grad, float* loss_rows, float* logprobs,
                  int64_t ldp, int32_t* argmax, const float* row_mask, int32_t masked_class, int32_t* labels);

/* The per-row part of the above for rows of ANY width, from the statistics nm_row_stats (nmhip.h) left in rmax / rlse /
 * argmax: loss_rows as above (reads x[r*ld + t]); weights[r] = 1 where the target is neither pad_id nor outside
 * [0, K), else 0 -- the row weights nm_xent takes for the gradient; labels as above.  Every output may be NULL;
 * targets NULL skips loss and weights. */
int nm_label_rows_from_stats(void* stream, const float* logits, int64_t ld, int64_t rows, int64_t K,
                             const int32_t* targets, int32_t pad_id, const float* rmax, const float* rlse,
                             float* loss_rows, float* weights, const int32_t* argmax, const float* row_mask,
                             int32_t masked_class, int32_t* labels);

#ifdef __cplusplus
}
#endif
#endif
