/* libnmhip -- C ABI of the frozen ImageNet networks (csrc/nm_vgg.hip), a companion of nmhip.h and nmhip_image.h with
 * the same conventions: every function returns 0 on success, <0 on error with the text in nm_last_error(); tensor
 * pointers are DEVICE pointers owned by the caller (fp32); `stream` is a hipStream_t passed as void*; sizes and leading
 * dimensions are int64_t element counts.  Arguments are checked before anything is launched.  No kernel here uses
 * floating-point atomics: two runs are bit-equal.
 *
 * Reference: neuralmonkey/encoders/imagenet_encoder.py, whose networks are TF-slim's (nets/vgg.py: every layer a
 * slim.conv2d, i.e. convolution + bias + ReLU).  Maps are NHWC, x[((b*H + y)*W + x)*ldx + c] with unit channel stride
 * and ldx >= C; filters are TensorFlow's [k, k, Cin, Cout], contiguous.  NM_PAD_VALID / NM_PAD_SAME are
 * nmhip_image.h's: 0 VALID (the output has H - k + 1 rows), 1 SAME (the output has the input's size; of the k - 1
 * padded rows (k - 1) / 2 lie before the map, as TensorFlow places them). */
#ifndef NMHIP_VGG_H
#define NMHIP_VGG_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* slim.conv2d(x, Cout, [k, k], padding=..., activation_fn=relu or None) at stride 1, forward only (the reference stops
 * the gradient behind the network, imagenet_encoder.py:212, :234):
 *   y[b, oy, ox, co] = act(bias[co] + sum_{ky, kx, ci} x[b, oy + ky - pt, ox + kx - pl, ci] * filt[ky, kx, ci, co])
 * with positions outside the map read as zero, act = max(., 0) when relu != 0; bias may be NULL (no bias); y is
 * [B, OH, OW, Cout] with rows of ldy floats.  An implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32) whose M dimension
 * runs over the FLATTENED output positions (image, row, column) and whose K dimension runs over the flattened
 * (ky, kx, ci) of the filter, so tiles are full whatever the map's width and Cin = 3 is one short K of 27.
 * algo: 0 auto, 1 tiles of 128 positions x 64 channels, 2 of 64 x 64.
 * Refused: B, H, W, Cin, Cout, k < 1; k > 7; VALID with H < k or W < k; more than 2^31 - 1 elements in a map or the
 * filter; ldx < Cin, ldy < Cout; a null x, filt or y; y overlapping x; a padding or algo outside the lists. */
int nm_conv2d_act_fwd(void* stream, const float* x, int64_t ldx, int64_t B, int64_t H, int64_t W, int64_t Cin,
                      const float* filt, int64_t k, int64_t Cout, int padding, const float* bias, int relu, float* y,
                      int64_t ldy, int algo);

#ifdef __cplusplus
}
#endif
#endif
