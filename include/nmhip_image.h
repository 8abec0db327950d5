/* libnmhip -- C ABI of the image stack (csrc/nm_image.hip), a companion of nmhip.h with the same conventions: every
 * function returns 0 on success, <0 on error with the text in nm_last_error(); tensor pointers are DEVICE pointers owned
 * by the caller (fp32, or int32 where said); `stream` is a hipStream_t passed as void*; sizes and leading dimensions are
 * int64_t element counts.  Arguments are checked before anything is launched.  No kernel here uses floating-point
 * atomics: two runs are bit-equal.
 *
 * Reference: neuralmonkey/encoders/cnn_encoder.py.  Maps are NHWC, x[((b*H + y)*W + x)*ldx + c] with unit channel
 * stride and ldx >= C; filters are TensorFlow's [kh, kw, Cin, Cout] (square here, kh = kw = k), contiguous.
 * padding: 0 VALID (the output has H - k + 1 rows), 1 SAME (the output has the input's size at stride 1; of the k - 1
 * padded rows (k - 1) / 2 lie before the map and the rest after, as TensorFlow places them). */
#ifndef NMHIP_IMAGE_H
#define NMHIP_IMAGE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define NM_PAD_VALID 0
#define NM_PAD_SAME 1
#define NM_WINDOW_MAX 0
#define NM_WINDOW_AVG 1

/* tf.layers.conv2d(x, Cout, k, padding=..., activation=None) at stride 1 (cnn_encoder.py:231, :265, :273, :280):
 *   y[b, oy, ox, co] = bias[co] + sum_{ky, kx, ci} x[b, oy + ky - pt, ox + kx - pl, ci] * filt[ky, kx, ci, co]
 * with positions outside the map read as zero; y is [B, OH, OW, Cout] with rows of ldy floats.
 * algo: 0 auto, 1 the matrix-core kernel (exact fp32 v_mfma_f32_32x32x2_f32, k <= 7), 2 the scalar kernel (any k).
 * Refused: B, H, W, Cin, Cout, k < 1; VALID with H < k or W < k; more than 2^31 - 1 elements in a map; ldx < Cin,
 * ldy < Cout; a null x, filt, bias or y; y overlapping x; a padding or algo outside the lists; algo 1 with k > 7. */
int nm_conv2d_fwd(void* stream, const float* x, int64_t ldx, int64_t B, int64_t H, int64_t W, int64_t Cin,
                  const float* filt, int64_t k, int64_t Cout, int padding, const float* bias, float* y, int64_t ldy,
                  int algo);

/* Bytes of the workspace nm_conv2d_bwd needs for the filter and bias gradients of this shape (the fixed-order slabs of
 * the position slices); 0 for sizes the entry points refuse. */
int64_t nm_conv2d_workspace_bytes(int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t k, int64_t Cout, int padding);

/* The gradient of the convolution above (tf.gradients of the same lines) from dy [B, OH, OW, Cout], rows of lddy:
 *   dx[b, iy, ix, ci] (+)= sum_{ky, kx, co} dy[b, iy - ky + pt, ix - kx + pl, co] * filt[ky, kx, ci, co]   NULL: skipped
 *   dfilt [k, k, Cin, Cout] (+)= sum_{b, oy, ox} x[b, oy + ky - pt, ox + kx - pl, ci] * dy[b, oy, ox, co]   NULL: skipped
 *   dbias [Cout]            (+)= sum_{b, oy, ox} dy[b, oy, ox, co]                                        NULL: skipped
 * accumulate_dx / accumulate_params != 0 add into what is there.  The sums over positions run in a fixed order: slices
 * of positions into the workspace, then the slices one after the other.  workspace: nm_conv2d_workspace_bytes bytes,
 * needed with dfilt or dbias.  algo as above (1: the data and filter gradients on the matrix cores).
 * Refused: the sizes, padding and algo as above; ldx, lddx < Cin; lddy < Cout; a null x, filt or dy; dx overlapping dy;
 * dfilt or dbias without a workspace, or with one that is too small. */
int nm_conv2d_bwd(void* stream, const float* x, int64_t ldx, int64_t B, int64_t H, int64_t W, int64_t Cin,
                  const float* filt, int64_t k, int64_t Cout, int padding, const float* dy, int64_t lddy, float* dx,
                  int64_t lddx, int accumulate_dx, float* dfilt, float* dbias, int accumulate_params, void* workspace,
                  int64_t workspace_bytes, int algo);

/* tf.layers.batch_normalization(x, training=...) over the channel axis with TensorFlow's defaults, centre and scale
 * (cnn_encoder.py:107), optionally followed by the ReLU the reference applies after it (:236, :272, :279).  x, y are
 * [rows, C] with rows = B*H*W, leading dimensions ldx, ldy.
 *   training != 0: mean[c] and the BIASED variance var[c] of the rows (two passes: the mean, then the squared
 *     deviations), written to batch_mean / batch_var [C] (both required);
 *     y = gamma * (x - mean) / sqrt(var + eps) + beta, then max(., 0) when relu != 0;
 *     when moving_mean and moving_var are given (both or neither) they are updated in place:
 *     moving = momentum * moving + (1 - momentum) * batch, where the variance that enters the moving variance is the
 *     UNBIASED one, var * rows / max(rows - 1, 1), as TensorFlow 1.x's fused batch norm hands it on;
 *   training == 0: the same expression from moving_mean / moving_var (both required, not written); batch_mean and
 *     batch_var are ignored.
 * Refused: rows, C < 1; rows * C beyond 2^31 - 1; ldx, ldy < C; a null x, gamma, beta or y; missing statistics as
 * above; eps <= 0; momentum outside [0, 1]. */
int nm_bn2d_fwd(void* stream, const float* x, int64_t ldx, int64_t rows, int64_t C, const float* gamma,
                const float* beta, float eps, float momentum, int training, int relu, float* moving_mean,
                float* moving_var, float* batch_mean, float* batch_var, float* y, int64_t ldy);

/* The gradient of the training-mode batch norm above.  With g = dy where relu == 0, else dy where the saved output
 * y > 0 and 0 elsewhere, xhat = (x - mean) / sqrt(var + eps):
 *   sums[c] = sum_r g, sums[C + c] = sum_r g * xhat     (sums: [2C] scratch, written whole, fixed order)
 *   dbeta (+)= sums[:C]; dgamma (+)= sums[C:]            either may be NULL
 *   dx (+)= gamma / sqrt(var + eps) * (g - sums[c] / rows - xhat * sums[C + c] / rows)     dx may be NULL
 * dx may be dy itself (each element is read before it is written) but must not overlap it otherwise.
 * Refused: the sizes as above; a null x, dy, gamma, batch_mean, batch_var or sums; relu != 0 without y; leading
 * dimensions below C; dx partially overlapping dy. */
int nm_bn2d_bwd(void* stream, const float* x, int64_t ldx, const float* y, int64_t ldy, const float* dy, int64_t lddy,
                int64_t rows, int64_t C, const float* gamma, const float* batch_mean, const float* batch_var, float eps,
                int relu, float* dx, int64_t lddx, int accumulate_dx, float* dgamma, float* dbeta,
                int accumulate_params, float* sums);

/* tf.layers.max_pooling2d / average_pooling2d (cnn_encoder.py:318-319), the pooling of the mask (:238, :319; C = 1,
 * no gradient) and, with the window (H, W) in average mode, tf.reduce_mean(x, [1, 2]) (:187).  Window (kh, kw), stride
 * (sh, sw); VALID: OH = (H - kh) / sh + 1; SAME: OH = ceil(H / sh), of the max((OH - 1) sh + kh - H, 0) padded rows half
 * (rounded down) lie before the map; padded positions take no part (the average divides by the positions inside).
 * mode NM_WINDOW_MAX: the FIRST maximum in row-major window order wins; argmax (int32 [B, OH, OW, C], contiguous, may
 * be NULL) receives its iy * W + ix for nm_window2d_bwd.  y is [B, OH, OW, C] with rows of ldy.
 * Refused: sizes, windows or strides < 1; VALID with H < kh or W < kw; a map beyond 2^31 - 1 elements; ldx, ldy < C; a
 * null x or y; y overlapping x; an unknown padding or mode. */
int nm_window2d_fwd(void* stream, const float* x, int64_t ldx, int64_t B, int64_t H, int64_t W, int64_t C, int64_t kh,
                    int64_t kw, int64_t sh, int64_t sw, int padding, int mode, float* y, int64_t ldy, int32_t* argmax);

/* The gradient of the pooling above: every input position gathers from the windows that hold it, in row-major order of
 * the windows (no atomics).  Max: dy of the windows whose argmax it is (argmax required); average: dy / (positions of
 * the window inside the map).  dx [B, H, W, C] rows of lddx, every element written (accumulate != 0: added to).
 * Refused: as above; a null dy or dx; max mode without argmax; dx overlapping dy. */
int nm_window2d_bwd(void* stream, const float* dy, int64_t lddy, const int32_t* argmax, int64_t B, int64_t H, int64_t W,
                    int64_t C, int64_t kh, int64_t kw, int64_t sh, int64_t sw, int padding, int mode, float* dx,
                    int64_t lddx, int accumulate);

/* The transpose behind CNNTemporalView.temporal_states (cnn_encoder.py:340-344: tf.transpose(x, [0, 2, 1, 3]) and the
 * reshape to [B, W, H*C]), both buffers contiguous: inverse == 0 writes dst[b, x, y*C + c] = src[b, y, x, c] from a map;
 * inverse != 0 writes the map dst[b, y, x, c] = src[b, x, y*C + c], which is also the gradient of the former.
 * Refused: sizes < 1; more than 2^31 - 1 elements; a null pointer; dst overlapping src. */
int nm_map_columns(void* stream, const float* src, float* dst, int64_t B, int64_t H, int64_t W, int64_t C, int inverse);

#ifdef __cplusplus
}
#endif
#endif
