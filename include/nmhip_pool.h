/* libnmhip -- C ABI of the sentence-level heads (csrc/nm_pool.hip), a companion of nmhip.h with the same conventions:
 * every function returns 0 on success, <0 on error with the text in nm_last_error(); tensor pointers are DEVICE pointers
 * owned by the caller (fp32 / int32); `stream` is a hipStream_t passed as void*; sizes and leading dimensions are
 * int64_t element counts.  Arguments are checked before anything is launched.  No kernel here uses floating-point
 * atomics: two runs are bit-equal.
 *
 * Reference: neuralmonkey/encoders/pooling.py, encoders/attentive.py, decoders/sequence_regressor.py.  States are
 * batch-major x[(b*T + t)*ldx + d], b < B, t < T, d < D with unit feature stride and ldx >= D (encoders hand out column
 * slices); mask is [B, T] float 0/1, contiguous. */
#ifndef NMHIP_POOL_H
#define NMHIP_POOL_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define NM_POOL_MAX 0     /* SequenceMaxPooling (pooling.py:44-51) */
#define NM_POOL_AVG 1     /* SequenceAveragePooling (pooling.py:60-63) */

/* Masked reduction over time, out[b*ldo + d]:
 *   NM_POOL_MAX  p = x*m + 1e-15f*(1 - m);  out = max_t p.  A padded position contributes 1e-15, not -inf: a column
 *                whose real values are all negative pools to 1e-15 when its sentence has padding.  ties[b*D + d]
 *                (int32, required) = how many of the T positions of p, padded ones included, equal the maximum -- the
 *                count the gradient of tf.reduce_max divides by.
 *   NM_POOL_AVG  out = sum_t(x*m) / (sum_t m + 1e-8f); a sentence of length 0 gives exact zeros.  ties is not read.
 * Refused: a mode other than the two, B, T, D < 1, B*T or the grid beyond 2^31, ldx < D, ldo < D, a null pointer. */
int nm_pool_fwd(void* stream, int mode, const float* x, int64_t ldx, const float* mask, int64_t B, int64_t T, int64_t D,
                float* out, int64_t ldo, int32_t* ties);

/* Gradient of the above, every (b, t, d) written (exact zeros at padded positions), dx[(b*T + t)*lddx + d]:
 *   NM_POOL_MAX  dx (+)= m * dout * [p == out] / ties        (needs x, out and ties of the forward call)
 *   NM_POOL_AVG  dx (+)= m * dout / (sum_t m + 1e-8f)        (x, out, ties are not read and may be NULL)
 * accumulate != 0 adds into dx.  dx must not overlap x.  Refused as above, plus lddo < D, lddx < D. */
int nm_pool_bwd(void* stream, int mode, const float* x, int64_t ldx, const float* mask, const float* out, int64_t ldo,
                const int32_t* ties, const float* dout, int64_t lddo, int64_t B, int64_t T, int64_t D, float* dx,
                int64_t lddx, int accumulate);

/* attentive.py:60-75 on energies e[(b*T + t)*lde + h], h < H heads, normalised along T in their natural layout:
 *   s = softmax_t(e) over all T positions, padded ones included (the maximum over all T is subtracted)
 *   u = s*m;  Z = sum_t u + 1e-8f;  w = u / Z                 mask NULL: w = s, Z = 1
 * w [B, T, H] with row stride ldw; s_out [B, T, H] (row stride lds, or NULL) and z_out [B, H] (or NULL) are what
 * nm_time_softmax_bwd reads.  w may be e itself (in place).  Refused: B, T, H < 1, lde / ldw / lds < H, null e or w. */
int nm_time_softmax_fwd(void* stream, const float* e, int64_t lde, const float* mask, int64_t B, int64_t T, int64_t H,
                        float* w, int64_t ldw, float* s_out, int64_t lds, float* z_out);

/* ... and its gradient from dw [B, T, H] (row stride lddw), s and Z of the forward call:
 *   du = dw/Z - sum_t(dw*u)/Z^2;  ds = du*m;  de (+)= s*(ds - sum_t ds*s)          mask NULL: ds = dw (z is not read)
 * de may be dw itself (in place, without accumulate). */
int nm_time_softmax_bwd(void* stream, const float* dw, int64_t lddw, const float* s, int64_t lds, const float* z,
                        const float* mask, int64_t B, int64_t T, int64_t H, float* de, int64_t ldde, int accumulate);

/* sequence_regressor.py:76-79 per row: loss_rows[r] = sum_k (p[r*ld + k] - y[r])^2 (or NULL); write_grad: p <-
 * scale * 2 (p - y) IN PLACE, scale one DEVICE float (NULL = 1) -- the counterpart of nm_label_rows' write_grad.
 * Refused: dim < 1, ld < dim, rows < 0, null pred or targets.  rows == 0 is a no-op. */
int nm_sqerr_rows(void* stream, float* pred, int64_t ld, int64_t rows, int64_t dim, const float* targets,
                  const float* grad_scale, int write_grad, float* loss_rows);

#ifdef __cplusplus
}
#endif
#endif
