/* libnmhip -- C ABI of the streaming scaled dot-product attention kernels (csrc/nm_sdp_stream.hip), a
 * companion of nmhip.h with the same conventions: every function returns 0 on success, <0 on error with the text in
 * nm_last_error(); tensor pointers are DEVICE pointers owned by the caller (fp32); `stream` is a hipStream_t passed as
 * void*; sizes and strides are int64_t element counts.  Arguments are checked before anything is launched.
 *
 * The arithmetic is that of nm_sdp_attn_fwd / nm_sdp_attn_bwd (nmhip.h): energies (q / sqrt(dh)) . k^T per head, the
 * causal where(j <= i + Tk - Tq, e, -1e9), the key mask e * m + (1 - m) * -1e9, softmax, the counter-based dropout over
 * the flat [Bq, H, Tq, Tk] index (salt, optional device scalar `step`), then . v.  Query row r reads key batch
 * r / rows_per_key; batch strides may exceed T * H * dh (cache views).  The difference is where the keys live: these
 * kernels stream key / value tiles of 64 positions through LDS and carry the softmax online, so Tq and Tk are not bound
 * by LDS, and the backward pass recomputes the weights from the saved row maximum and row sum instead of reading a
 * [Bq, H, Tq, Tk] tensor back.  fp32 on v_mfma_f32_16x16x4_f32; head widths 16, 32, 64, 128.  No atomics: two runs are
 * bit-equal.
 *
 * Refused by both entry points: null pointers (key_mask, step, weights, row_max / row_sum of the forward excepted),
 * non-positive sizes, Bq % rows_per_key, dh outside {16, 32, 64, 128}, q / k / v / ctx / dctx / dq / dk / dv off 16-byte
 * alignment or with a batch stride that is no multiple of 4 floats, keep_prob outside (0, 1], Bq H Tq Tk >= 2^32 when
 * keep_prob < 1 (the dropout index), Bq * H >= 2^31 or more than 65535 * 64 positions (the grid); rows_per_key != 1 in
 * the backward. */
#ifndef NMHIP_SDP_STREAM_H
#define NMHIP_SDP_STREAM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* 1 where nm_sdp_attn_fwd refuses (Tq, Tk, dh) for lack of LDS and, with backward != 0, also where nm_sdp_attn_bwd
 * does; 0 otherwise (the resident kernels take the shape and keep it). */
int nm_sdp_stream_wanted(int64_t Tq, int64_t Tk, int64_t dh, int backward);

/* bytes of the backward's workspace: D[b, h, i] = dctx_i . ctx_i, Bq * H * Tq floats */
int64_t nm_sdp_stream_workspace_bytes(int64_t Bq, int64_t H, int64_t Tq);

/* Operands as nm_sdp_attn_fwd.  weights [Bq, H, Tq, Tk] (the softmax output before dropout) or null; row_max / row_sum
 * [Bq, H, Tq]: the maximum of a row's masked energies and the sum of exp(e - max) over its keys, both or neither (null
 * when no backward will follow).  Tq == 1 with keep_prob == 1 and no row_max goes to the one-query kernel of
 * nm_sdp_attn_fwd. */
int nm_sdp_stream_fwd(void* stream, const float* q, int64_t q_bs, const float* k, int64_t k_bs, const float* v,
                      int64_t v_bs, const float* key_mask, int64_t mask_bs, int64_t Bq, int64_t rows_per_key,
                      int64_t Tq, int64_t Tk, int64_t H, int64_t dh, int causal, float keep_prob, uint32_t salt,
                      const uint32_t* step, float* ctx, int64_t ctx_bs, float* weights, float* row_max,
                      float* row_sum);

/* ctx, row_max, row_sum: what the forward wrote for the same operands, salt and step.  dq / dk / dv are written, or
 * added to with accumulate != 0.  workspace: nm_sdp_stream_workspace_bytes(B, H, Tq) bytes. */
int nm_sdp_stream_bwd(void* stream, const float* q, int64_t q_bs, const float* k, int64_t k_bs, const float* v,
                      int64_t v_bs, const float* key_mask, int64_t mask_bs, const float* ctx, int64_t ctx_bs,
                      const float* row_max, const float* row_sum, const float* dctx, int64_t dctx_bs, int64_t B,
                      int64_t rows_per_key, int64_t Tq, int64_t Tk, int64_t H, int64_t dh, int causal,
                      float keep_prob, uint32_t salt, const uint32_t* step, float* dq, int64_t dq_bs, float* dk,
                      int64_t dk_bs, float* dv, int64_t dv_bs, float* workspace, int accumulate);

#ifdef __cplusplus
}
#endif
#endif
