/* libnmhip -- C ABI of the image reader's device pipeline (csrc/nm_imgread.hip), a companion of nmhip.h with the same
 * conventions: every function returns 0 on success, <0 on error with the text in nm_last_error(); pointers are DEVICE
 * pointers owned by the caller; `stream` is a hipStream_t passed as void*; sizes are int64_t counts.  Arguments are
 * checked before anything is launched.  No atomics: two runs are bit-equal, and an image's output does not depend on
 * what else is in the chunk.
 *
 * The arithmetic is Pillow's (Image.convert, Image.resize with the BILINEAR and BICUBIC filters, Image.crop) followed by
 * the zero padding of the reference's readers/image_reader.py:_pad; the tables are Pillow's precompute_coeffs, made on
 * the host in float64.  A ragged chunk of N decoded 8-bit images (1 band "L" or 3 bands "RGB", rows top to bottom) is
 *   src     one byte array, image i at the bytes offs[0][i] .. offs[0][i+1]
 *   offs    int64 [NM_IMGREAD_OFFS][N + 1]: row 0 bytes into src, 1 elements into scratch, 2 / 3 entries into bounds /
 *           coef of the horizontal table, 4 / 5 the same of the vertical table
 *   geom    int32 [N][NM_IMGREAD_GEOM]: 0 source width, 1 source height, 2 bands, 3 resized width, 4 resized height,
 *           5 crop x, 6 crop y, 7 copied width cw, 8 copied height ch, 9 first source row the vertical pass reads,
 *           10 number of such rows, 11 taps per output of the horizontal table (ksize), 12 of the vertical table
 *   bounds  int32 pairs (first input index, tap count), one per kept output: the horizontal table of image i has cw
 *           pairs -- the outputs crop x .. crop x + cw of the resize, so cropped-away columns are never computed -- the
 *           vertical one ch pairs
 *   coef    ksize numbers per pair: int32 (Pillow's 22-bit fixed point) for the targets L and RGB, float64 for F
 * A pass that Pillow would skip has the one-tap table (first = the output's own index, count 1, coefficient 1).
 * Everything read on the device is clamped before it becomes an address: indices outside their array read as 0, and a
 * scratch or output element that no image's geometry covers is written as 0 (output) or not at all (scratch). */
#ifndef NMHIP_IMGREAD_H
#define NMHIP_IMGREAD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define NM_IMGREAD_L 0
#define NM_IMGREAD_RGB 1
#define NM_IMGREAD_F 2
#define NM_IMGREAD_OFFS 6
#define NM_IMGREAD_GEOM 16
#define NM_IMGREAD_MAX_IMAGES 65535

/* Horizontal pass with the conversion to `target` folded into the loads:
 *   RGB -> L  (19595 R + 38470 G + 7471 B + 0x8000) >> 16        RGB -> F  float(299 R + 587 G + 114 B) / 1000.0f
 *   L -> RGB  replicated                                          L -> F    the value
 * For source row geom[9] + r (r < geom[10]), kept column x and channel c
 *   L, RGB  scratch[offs[1][i] + (r*cw + x)*C + c] = clip((2^21 + sum_t pixel(first + t) * coef[t]) >> 22, 0, 255)   uint8
 *   F       the same sum in float64, product rounded before the add, taps in order, rounded to float32 once
 * (C = 3 for RGB, else 1).  `pad_w` bounds every cw, `max_rows` every geom[10]: they size the grid.
 * Refused: null src, offs, geom, bounds, coef or scratch; N outside 1..65535; a target other than L, RGB, F; pad_w < 1;
 * max_rows < 0; negative src_bytes, scratch_elems, n_bounds or n_coef.  max_rows == 0 or src_bytes == 0 is a no-op.
 * (bands other than 1 or 3 are refused by nm_imgread_check, which sees the host's copy of geom.) */
int nm_imgread_rows(void* stream, const void* src, int64_t src_bytes, const int64_t* offs, const int32_t* geom, int64_t N,
                    const int32_t* bounds, int64_t n_bounds, const void* coef, int64_t n_coef, int target, int64_t pad_w,
                    int64_t max_rows, void* scratch, int64_t scratch_elems);

/* Vertical pass over the scratch, crop, zero padding and the optional epilogue: for image i, row y < pad_h, column
 * x < pad_w, channel c
 *   v = y < ch and x < cw ? the vertical sum over scratch rows (first - geom[9]) + t : 0
 *   out[(i*pad_h + y)*ld + x*C + c] = float(v), or float((double(v) - sub[c]) / divide) when sub is given or divide != 1
 * (the epilogue also covers the padding, as the reference's imagenet_reader subtracts from the padded array).
 * Refused: null scratch, offs, geom, bounds, coef or out; N outside 1..65535; a target other than L, RGB, F; pad_w or
 * pad_h < 1; ld < pad_w * C; N * pad_h * ld beyond 2^31 - 1; divide == 0; negative scratch_elems, n_bounds, n_coef. */
int nm_imgread_cols(void* stream, const void* scratch, int64_t scratch_elems, const int64_t* offs, const int32_t* geom,
                    int64_t N, const int32_t* bounds, int64_t n_bounds, const void* coef, int64_t n_coef, int target,
                    int64_t pad_w, int64_t pad_h, const double* sub, double divide, float* out, int64_t ld);

/* The HOST copies of a chunk's geom and offs, checked before they are uploaded (host pointers): bands other than 1 or
 * 3, negative extents, cw > pad_w or ch > pad_h, offsets that decrease or an image whose bytes, scratch or tables do not
 * fit between its offsets are refused with the image's index in the text. */
int nm_imgread_check(const int64_t* host_offs, const int32_t* host_geom, int64_t N, int target, int64_t pad_w,
                     int64_t pad_h);

#ifdef __cplusplus
}
#endif
#endif
