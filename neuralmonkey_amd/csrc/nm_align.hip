// Supervised attention (include/nmhip_align.h): the rows of decoders/word_alignment_decoder.py --
// tf.nn.softmax_cross_entropy_with_logits(labels = the reference alignment, logits = the attention WEIGHTS of the
// teacher-forced steps) * train_padding (:100-108), the gradient TensorFlow 1.12 registers for that op, and the runtime
// tf.nn.softmax of the recorded weights, batch-major (:91-97).
//
//   align_xent_kernel      one wavefront per (t, b) row, four rows per workgroup; lanes stride over the S source
//                          positions.  Each lane keeps its first position (all of the row up to S = 64: the reference's
//                          sentences) in registers, further trips re-read the row from cache.  Row maximum, sum exp,
//                          sum label and sum label * w are 64-wide shuffle reductions -- no LDS, no barrier, no atomics.
//                          The label row is read in place from the batch-major fed array through its two strides.
//                          Lane 0 writes the row's loss; with ``dw`` every lane writes (or adds) its positions of
//                          scale * pad * (softmax(w) - label).
//   align_softmax_kernel   the same row layout: out[b, t, :] = softmax(w[t, b, :]).
#include "nm_common.h"

namespace {

constexpr int ALIGN_WAVES = 4;               // rows per workgroup

// max and sum exp(x - max) of one row, lanes striding over it; ``first`` is the lane's own position 0 (s = lane)
__device__ __forceinline__ void align_row_stats(const float* __restrict__ wr, long S, int lane, float first, float& m,
                                                float& sum) {
    float mx = lane < S ? first : -INFINITY;
    for (long s = lane + 64; s < S; s += 64) mx = fmaxf(mx, wr[s]);
    m = nm_wave_max(mx);
    float acc = lane < S ? expf(first - m) : 0.0f;
    for (long s = lane + 64; s < S; s += 64) acc += expf(wr[s] - m);
    sum = nm_wave_sum(acc);
}

__global__ __launch_bounds__(64 * ALIGN_WAVES) void align_xent_kernel(
    const float* __restrict__ w, long T, long B, long S, const float* __restrict__ target, long sb, long st,
    const float* __restrict__ pad, const float* __restrict__ scale, float* __restrict__ loss_rows, float* dw,
    int accumulate) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * ALIGN_WAVES + (threadIdx.x >> 6);
    if (r >= T * B) return;                                        // wave-uniform: the shuffles below see full waves
    const float p = pad[r];
    float* dr = dw != nullptr ? dw + r * S : nullptr;
    if (p == 0.0f) {                                               // a padded target position: exact zeros, label unread
        if (lane == 0) loss_rows[r] = 0.0f;
        if (dr != nullptr && !accumulate)
            for (long s = lane; s < S; s += 64) dr[s] = 0.0f;
        return;
    }
    const long t = r / B, b = r - t * B;
    const float* wr = w + r * S;
    const float* lr = target + b * sb + t * st;
    const float w0 = lane < S ? wr[lane] : 0.0f;
    const float l0 = lane < S ? lr[lane] : 0.0f;
    float m, sum;
    align_row_stats(wr, S, lane, w0, m, sum);
    float sl = l0, slw = l0 * w0;
    for (long s = lane + 64; s < S; s += 64) {
        const float l = lr[s];
        sl += l;
        slw = fmaf(l, wr[s], slw);
    }
    sl = nm_wave_sum(sl);
    slw = nm_wave_sum(slw);
    if (lane == 0) loss_rows[r] = p * (sl * (m + logf(sum)) - slw);
    if (dr == nullptr) return;
    const float g = (scale != nullptr ? scale[0] : 1.0f) * p;
    const float inv = 1.0f / sum;
    if (lane < S) {
        const float d = g * (expf(w0 - m) * inv - l0);
        dr[lane] = accumulate ? dr[lane] + d : d;
    }
    for (long s = lane + 64; s < S; s += 64) {
        const float d = g * (expf(wr[s] - m) * inv - lr[s]);
        dr[s] = accumulate ? dr[s] + d : d;
    }
}

__global__ __launch_bounds__(64 * ALIGN_WAVES) void align_softmax_kernel(const float* __restrict__ w, long T, long B,
                                                                         long S, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * ALIGN_WAVES + (threadIdx.x >> 6);
    if (r >= T * B) return;
    const long t = r / B, b = r - t * B;
    const float* wr = w + r * S;
    float* orow = out + (b * T + t) * S;
    const float w0 = lane < S ? wr[lane] : 0.0f;
    float m, sum;
    align_row_stats(wr, S, lane, w0, m, sum);
    const float inv = 1.0f / sum;
    if (lane < S) orow[lane] = expf(w0 - m) * inv;
    for (long s = lane + 64; s < S; s += 64) orow[s] = expf(wr[s] - m) * inv;
}

// the size checks the two entry points share; 1 = nothing to do
int align_sizes(const char* fn, int64_t T, int64_t B, int64_t S, int* empty) {
    NM_REQUIRE(T >= 0 && B >= 0 && S >= 0, "%s: bad sizes T %lld, B %lld, S %lld", fn, (long long)T, (long long)B,
               (long long)S);
    const int64_t lim = (1ll << 31) - 1;
    NM_REQUIRE(T == 0 || B == 0 || (T <= lim && B <= lim && T * B <= lim), "%s: T*B = %lld x %lld rows beyond 2^31 - 1",
               fn, (long long)T, (long long)B);
    *empty = T * B == 0;
    NM_REQUIRE(*empty || S >= 1, "%s: S = %lld source positions with %lld rows, at least 1 is needed", fn, (long long)S,
               (long long)(T * B));
    return NM_OK;
}

}  // namespace

extern "C" {

int nm_align_xent(void* stream, const float* w, int64_t T, int64_t B, int64_t S, const float* target,
                  int64_t tgt_stride_b, int64_t tgt_stride_t, const float* pad, const float* scale, float* loss_rows,
                  float* dw, int accumulate) {
    int empty = 0;
    if (int rc = align_sizes("nm_align_xent", T, B, S, &empty)) return rc;
    if (empty) return NM_OK;
    NM_REQUIRE(w != nullptr && target != nullptr && pad != nullptr && loss_rows != nullptr,
               "nm_align_xent: null pointer (w, target, pad or loss_rows)");
    NM_REQUIRE(tgt_stride_t >= S, "nm_align_xent: tgt_stride_t %lld below S %lld (label rows would overlap)",
               (long long)tgt_stride_t, (long long)S);
    NM_REQUIRE(tgt_stride_b / T >= tgt_stride_t, "nm_align_xent: tgt_stride_b %lld below T * tgt_stride_t = %lld x %lld "
               "(sentences would overlap)", (long long)tgt_stride_b, (long long)T, (long long)tgt_stride_t);
    NM_REQUIRE(dw == nullptr || dw != w, "nm_align_xent: dw aliasing w");
    hipLaunchKernelGGL(align_xent_kernel, dim3((unsigned)nm_cdiv(T * B, ALIGN_WAVES)), dim3(64 * ALIGN_WAVES), 0,
                       nm_stream(stream), w, (long)T, (long)B, (long)S, target, (long)tgt_stride_b, (long)tgt_stride_t,
                       pad, scale, loss_rows, dw, accumulate ? 1 : 0);
    NM_LAUNCH_CHECK("nm_align_xent");
}

int nm_align_softmax(void* stream, const float* w, int64_t T, int64_t B, int64_t S, float* out) {
    int empty = 0;
    if (int rc = align_sizes("nm_align_softmax", T, B, S, &empty)) return rc;
    if (empty) return NM_OK;
    NM_REQUIRE(w != nullptr && out != nullptr, "nm_align_softmax: null pointer (w or out)");
    NM_REQUIRE(out != w, "nm_align_softmax: out aliasing w (the rows change places)");
    hipLaunchKernelGGL(align_softmax_kernel, dim3((unsigned)nm_cdiv(T * B, ALIGN_WAVES)), dim3(64 * ALIGN_WAVES), 0,
                       nm_stream(stream), w, (long)T, (long)B, (long)S, out);
    NM_LAUNCH_CHECK("nm_align_softmax");
}

}  // extern "C"
