/* libnmhip -- C ABI of the convolutional sequence-to-sequence encoder's residual layer (csrc/nm_conv.hip), a companion
 * of nmhip.h with the same conventions: every function returns 0 on success, <0 on error with the text in
 * nm_last_error(); tensor pointers are DEVICE pointers owned by the caller (fp32); `stream` is a hipStream_t passed as
 * void*; sizes and leading dimensions are int64_t element counts.  Arguments are checked before anything is launched.
 * No kernel here uses floating-point atomics: two runs are bit-equal.
 *
 * Reference: neuralmonkey/encoders/facebook_conv.py (Gehring et al. 2017), nn/projection.py.  States are batch-major
 * x[(b*T + t)*ldx + c], b < B, t < T, c < C with unit feature stride and ldx >= C; the filter is TensorFlow's conv1d
 * filter W[(k*C + e)*2C + o], k < w taps, e < C input channels, o < 2C: column c is the linear half, column C + c its
 * gate; bias [2C] likewise.  SAME padding: (w - 1) / 2 zero positions before the sentence, the rest after. */
#ifndef NMHIP_CONVS2S_H
#define NMHIP_CONVS2S_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* One residual layer, facebook_conv.py:102-121 (tf.nn.conv1d(x, W, 1, "SAME") + bias, then glu(.) + x) with
 * nn/projection.py:60-75 (glu: the first half times the sigmoid of the second):
 *   lin  = sum_{k, e} x[b, t + k - (w-1)/2, e] * W[k, e, c]     + bias[c]
 *   gate = sum_{k, e} x[b, t + k - (w-1)/2, e] * W[k, e, C + c] + bias[C + c]
 *   y[(b*T + t)*ldy + c] = lin * sigmoid(gate) + x[b, t, c]
 * Positions outside [0, T) read as zero; nothing is masked, as in the reference.  lin_save / sig_save: contiguous
 * [B*T, C] buffers that receive lin and sigmoid(gate) for nm_conv1d_glu_bwd -- both (training) or both NULL
 * (inference); y is bit-identical in the two modes.  algo: 0 auto, 1 the matrix-core kernel (w <= 8), 2 the scalar kernel
 * (any width); auto takes the scalar kernel where w > 8.  No [B, T, 2C] pre-activation is written.
 * Refused: B, T, C, w < 1; B*T or the grid beyond 2^31; ldx < C, ldy < C; a null x, W, bias or y; y overlapping x (a
 * tile reads its neighbours' rows of x as halo); exactly one of the two save pointers; an algo other than the three;
 * algo 1 with w > 8. */
int nm_conv1d_glu_fwd(void* stream, const float* x, int64_t ldx, int64_t B, int64_t T, int64_t C, int64_t w,
                      const float* W, const float* bias, float* y, int64_t ldy, float* lin_save, float* sig_save,
                      int algo);

/* Bytes of the workspace nm_conv1d_glu_bwd needs for the weight gradient of this shape (the fixed-order slabs of the
 * position slices); 0 for sizes the entry points refuse. */
int64_t nm_conv1d_glu_workspace_bytes(int64_t B, int64_t T, int64_t C, int64_t w);

/* The gradient of the layer above (tf.gradients of facebook_conv.py:118-121) from dy[(b*T + t)*lddy + c] and the saved
 * lin / sigmoid(gate):
 *   dz [B*T, 2C] (contiguous scratch, written whole):  dz[:, :C] = dy * sig;  dz[:, C:] = dy * lin * sig * (1 - sig)
 *   dx[(b*T + t)*lddx + c] (+)= dy + conv1d^T(dz, W)    the residual term included; accumulate_dx != 0 adds into dx;
 *                                                       dx may be NULL (no input gradient wanted)
 *   dW [w, C, 2C] (+)= sum_{b, t} x[b, t + k - (w-1)/2, e] * dz[b, t, o]        NULL: not computed
 *   dbias [2C]    (+)= sum_{b, t} dz[b, t, o]                                   NULL: not computed
 * accumulate_params != 0 adds into dW and dbias.  workspace: nm_conv1d_glu_workspace_bytes bytes, needed with dW.  The
 * sums run in a fixed order.  dx must not overlap dy.  algo as above (1: every kernel on the matrix cores, w <= 8).
 * Refused: the sizes and algo as above; ldx, lddy, lddx < C; a null x, W, lin_save, sig_save, dy or dz; dx overlapping
 * dy; dW without a workspace or with one that is too small. */
int nm_conv1d_glu_bwd(void* stream, const float* x, int64_t ldx, int64_t B, int64_t T, int64_t C, int64_t w,
                      const float* W, const float* lin_save, const float* sig_save, const float* dy, int64_t lddy,
                      float* dz, float* dx, int64_t lddx, int accumulate_dx, float* dW, float* dbias,
                      int accumulate_params, void* workspace, int64_t workspace_bytes, int algo);

#ifdef __cplusplus
}
#endif
#endif
