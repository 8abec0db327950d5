/* libnmhip -- C ABI of the batch norm whose statistics span the ranks of a data-parallel job (csrc/nm_bnsync.hip), a
 * companion of nmhip_image.h with the same conventions: every function returns 0 on success, <0 on error with the text
 * in nm_last_error(); tensor pointers are DEVICE pointers owned by the caller (fp32, or double where said); `stream` is
 * a hipStream_t passed as void*; sizes and leading dimensions are int64_t element counts.  Arguments are checked before
 * anything is launched.  No kernel here uses floating-point atomics: two runs are bit-equal.
 *
 * nm_bn2d_fwd / nm_bn2d_bwd (nmhip_image.h) take their statistics and their two channel sums from the rows they are
 * handed.  When a batch is dealt over several ranks, tf.layers.batch_normalization(x, training=True)
 * (neuralmonkey/encoders/cnn_encoder.py:107) over the WHOLE batch is these four steps around two exchanges:
 *   forward:  nm_bn2d_part_stats -> all ranks' parts gathered in rank order -> nm_bn2d_merge -> nm_bn2d_fwd with
 *             training == 0 on the merged batch_mean / batch_var (the same expression, nothing written to them)
 *   backward: nm_bn2d_bwd_sums -> the [2C] sums added over the ranks -> nm_bn2d_bwd_dx with the global row count
 * With one part the results are bit-equal to nm_bn2d_fwd (training != 0) and nm_bn2d_bwd.
 *
 * A part is NM_BN2D_PART_DOUBLES(C) = 2C + 1 doubles: [0] the row count (exact: a double holds every integer below
 * 2^53), [1 .. C] the channels' means, [C + 1 .. 2C] the channels' sums of squared deviations about those means (M2). */
#ifndef NMHIP_BNSYNC_H
#define NMHIP_BNSYNC_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define NM_BN2D_PART_DOUBLES(C) (2 * (C) + 1)

/* The part of this rank's rows x [rows, C] (leading dimension ldx), by the arithmetic of nm_bn2d_fwd: the column sums in
 * double, mean[c] = (float)(sum / rows) -- the rounded mean, stored widened -- then M2[c] = sum_r (x - mean[c])^2 in
 * double (two passes, never E[x^2] - E[x]^2).  part: NM_BN2D_PART_DOUBLES(C) doubles, all written.
 * Refused: rows, C < 1; rows * C beyond 2^31 - 1; ldx < C; a null x or part. */
int nm_bn2d_part_stats(void* stream, const float* x, int64_t ldx, int64_t rows, int64_t C, double* part);

/* The statistics of all rows from the parts of `world` ranks, parts[r * NM_BN2D_PART_DOUBLES(C) ...] being rank r's
 * (every part holds at least one row).  One thread per channel starts from part 0 and takes in parts 1, 2, ... in that
 * order, in double: with d = mean_r - mean,
 *   n' = n + n_r;   mean' = mean + d * n_r / n';   M2' = M2 + M2_r + d^2 * n * n_r / n'
 * and writes batch_mean[c] = (float)mean, the BIASED batch_var[c] = (float)(M2 / n) and total[0] = n (a double).  When
 * moving_mean and moving_var are given (both or neither) they are updated in place as nm_bn2d_fwd updates them:
 * moving = momentum * moving + (1 - momentum) * batch, the variance that enters the moving variance being the UNBIASED
 * one over the total count, var * n / max(n - 1, 1).  Every rank runs this on the same gathered parts in the same
 * order, which is what keeps the replicas' moving statistics bit-identical.
 * Refused: world, C < 1; C beyond 2^31 - 1; a null parts, batch_mean, batch_var or total; one moving pointer without the
 * other; momentum outside [0, 1]. */
int nm_bn2d_merge(void* stream, const double* parts, int64_t world, int64_t C, float momentum, float* moving_mean,
                  float* moving_var, float* batch_mean, float* batch_var, double* total);

/* The first half of nm_bn2d_bwd, from this rank's rows and the MERGED mean / var: with g = dy where relu == 0, else dy
 * where the saved output y > 0 and 0 elsewhere, xhat = (x - mean) / sqrt(var + eps):
 *   sums[c] = sum_r g, sums[C + c] = sum_r g * xhat       (sums: [2C], written whole, fixed order)
 *   dbeta (+)= sums[:C]; dgamma (+)= sums[C:]              either may be NULL; accumulate_params != 0 adds
 * These are the rank's OWN sums: the parameter gradients of the ranks are added up by the gradient exchange.
 * Refused: the sizes as above; a null x, dy, mean, var or sums; relu != 0 without y; ldx, lddy (ldy with relu) < C;
 * eps <= 0. */
int nm_bn2d_bwd_sums(void* stream, const float* x, int64_t ldx, const float* y, int64_t ldy, const float* dy,
                     int64_t lddy, int64_t rows, int64_t C, const float* mean, const float* var, float eps, int relu,
                     float* sums, float* dgamma, float* dbeta, int accumulate_params);

/* The second half, from the sums added over all ranks and the GLOBAL row count n:
 *   dx (+)= gamma / sqrt(var + eps) * (g - sums[c] / n - xhat * sums[C + c] / n)
 * dx may be dy itself (each element is read before it is written) but must not overlap it otherwise.
 * Refused: the sizes as above; a null x, dy, gamma, mean, var, sums or dx; relu != 0 without y; leading dimensions
 * below C; eps <= 0; n below rows; dx partially overlapping dy. */
int nm_bn2d_bwd_dx(void* stream, const float* x, int64_t ldx, const float* y, int64_t ldy, const float* dy, int64_t lddy,
                   int64_t rows, int64_t C, const float* gamma, const float* mean, const float* var, float eps, int relu,
                   const float* sums, int64_t n, float* dx, int64_t lddx, int accumulate_dx);

#ifdef __cplusplus
}
#endif
#endif
