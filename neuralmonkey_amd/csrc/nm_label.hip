// Sequence labelling head (include/nmhip_label.h): the rows of decoders/sequence_labeler.py -- tf.nn.log_softmax,
// tf.argmax, sparse_softmax_cross_entropy_with_logits * sentence_mask(targets) and the gradient of the logits -- for
// tag sets (tens of classes), where the vocabulary-row kernels of nm_logits.hip (one 1024-thread workgroup per row)
// would keep 4 % of their lanes busy and run three times over.
//
//   label_rows_kernel<NV>    one wavefront per row, four rows per workgroup; lane l holds classes l, l + 64, ... in NV
//                            registers (K <= 64 NV, NV <= 16).  The row is read from HBM once; max, argmax (first
//                            maximum wins), sum exp and the target's logit are reduced with 64-wide shuffles -- no LDS,
//                            no barrier, no atomics; loss, log-probabilities, argmax, masked labels and the in-place
//                            gradient are written straight from the registers.
//   label_from_stats_kernel  one thread per row: loss, 0/1 weights and masked labels from the row statistics of
//                            nm_row_stats, for rows wider than the packed kernel takes (ops.label_rows' fallback).
#include "nm_common.h"

namespace {

constexpr int LABEL_MAX_CLASSES = 1024;      // 16 registers of 64 lanes
constexpr int LABEL_WAVES = 4;               // rows per workgroup

template <int NV>
__global__ __launch_bounds__(64 * LABEL_WAVES) void label_rows_kernel(
    float* x, long ld, long rows, int K, const int32_t* __restrict__ targets, int pad_id,
    const float* __restrict__ grad_scale, int write_grad, float* __restrict__ loss_rows, float* logprobs, long ldp,
    int32_t* __restrict__ argmax, const float* __restrict__ row_mask, int masked_class, int32_t* __restrict__ labels) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * LABEL_WAVES + (threadIdx.x >> 6);
    if (r >= rows) return;                                         // wave-uniform: the shuffles below see full waves
    float* xr = x + r * ld;
    float d[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int k = lane + 64 * i;
        d[i] = k < K ? xr[k] : -INFINITY;
    }
    // maximum and its first index: ascending within the lane, (value, lower index) across the lanes; a lane without a
    // class of its own carries (-inf, index >= K), which loses every comparison against a real class
    float bv = d[0];
    int best = lane;
#pragma unroll
    for (int i = 1; i < NV; ++i)
        if (d[i] > bv) { bv = d[i]; best = lane + 64 * i; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off, 64);
        const int oi = __shfl_xor(best, off, 64);
        if (ov > bv || (ov == bv && oi < best)) { bv = ov; best = oi; }
    }
    const float m = bv;
    // the target's logit, before the registers turn into x - m: the lane that owns it selects it (no dynamic index)
    const bool has_t = targets != nullptr;
    const int t = has_t ? targets[r] : 0;
    const bool counted = has_t && t != pad_id;
    const bool in_range = t >= 0 && t < K;
    float xt = 0.0f;
    if (counted && in_range) {
        float cand = 0.0f;
#pragma unroll
        for (int i = 0; i < NV; ++i)
            if (i == (t >> 6)) cand = d[i];
        xt = __shfl(cand, t & 63, 64);
    }
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        d[i] -= m;                                                 // (-inf stays -inf: exp gives an exact 0)
        s += expf(d[i]);
    }
    s = nm_wave_sum(s);
    const float lse = logf(s);
    if (lane == 0) {
        if (has_t && loss_rows != nullptr) loss_rows[r] = !counted ? 0.0f : (in_range ? lse - (xt - m) : NAN);
        if (argmax != nullptr) argmax[r] = best;
        if (labels != nullptr) labels[r] = row_mask[r] != 0.0f ? best : masked_class;
    }
    if (logprobs != nullptr) {
        float* pr = logprobs + r * ldp;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int k = lane + 64 * i;
            if (k < K) pr[k] = d[i] - lse;
        }
    }
    if (write_grad) {
        if (counted && in_range) {
            const float sc = grad_scale != nullptr ? grad_scale[0] : 1.0f;
            const float inv = 1.0f / s;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int k = lane + 64 * i;
                if (k < K) xr[k] = sc * (expf(d[i]) * inv - (k == t ? 1.0f : 0.0f));
            }
        } else {                                                   // <pad> target, or one outside [0, K): exact zeros
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int k = lane + 64 * i;
                if (k < K) xr[k] = 0.0f;
            }
        }
    }
}

__global__ __launch_bounds__(256) void label_from_stats_kernel(
    const float* __restrict__ x, long ld, long rows, long K, const int32_t* __restrict__ targets, int pad_id,
    const float* __restrict__ rmax, const float* __restrict__ rlse, float* __restrict__ loss_rows,
    float* __restrict__ weights, const int32_t* __restrict__ argmax, const float* __restrict__ row_mask,
    int masked_class, int32_t* __restrict__ labels) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    if (targets != nullptr) {
        const int t = targets[r];
        const bool counted = t != pad_id, in_range = t >= 0 && t < K;
        if (loss_rows != nullptr)
            loss_rows[r] = !counted ? 0.0f : (in_range ? rlse[r] - (x[r * ld + t] - rmax[r]) : NAN);
        if (weights != nullptr) weights[r] = (counted && in_range) ? 1.0f : 0.0f;
    }
    if (labels != nullptr) labels[r] = row_mask[r] != 0.0f ? argmax[r] : masked_class;
}

}  // namespace

extern "C" {

int64_t nm_label_rows_max_classes(void) { return LABEL_MAX_CLASSES; }

int nm_label_rows(void* stream, float* logits, int64_t ld, int64_t rows, int64_t K, const int32_t* targets,
                  int32_t pad_id, const float* grad_scale, int write_grad, float* loss_rows, float* logprobs,
                  int64_t ldp, int32_t* argmax, const float* row_mask, int32_t masked_class, int32_t* labels) {
    NM_REQUIRE(K >= 1, "nm_label_rows: K = %lld classes, at least 1 is needed", (long long)K);
    NM_REQUIRE(K <= LABEL_MAX_CLASSES, "nm_label_rows: K = %lld classes above the packed kernel's maximum of %d",
               (long long)K, LABEL_MAX_CLASSES);
    NM_REQUIRE(rows >= 0 && rows < (1ll << 31) - LABEL_WAVES, "nm_label_rows: bad row count %lld", (long long)rows);
    NM_REQUIRE(ld >= K, "nm_label_rows: ld %lld below K %lld", (long long)ld, (long long)K);
    NM_REQUIRE(logprobs == nullptr || ldp >= K, "nm_label_rows: ldp %lld below K %lld", (long long)ldp, (long long)K);
    NM_REQUIRE(!write_grad || targets != nullptr, "nm_label_rows: write_grad without targets");
    NM_REQUIRE(labels == nullptr || row_mask != nullptr, "nm_label_rows: labels without row_mask");
    if (rows == 0) return NM_OK;
    NM_REQUIRE(logits != nullptr, "nm_label_rows: null pointer (logits)");
    if (logprobs != nullptr) {
        const float* x_end = logits + (rows - 1) * ld + K;
        const float* p_end = logprobs + (rows - 1) * ldp + K;
        NM_REQUIRE(p_end <= logits || x_end <= logprobs, "nm_label_rows: logprobs aliasing logits");
    }
    const dim3 grid((unsigned)nm_cdiv(rows, LABEL_WAVES)), block(64 * LABEL_WAVES);
#define NM_LR(NV_)                                                                                                   \
    hipLaunchKernelGGL((label_rows_kernel<NV_>), grid, block, 0, nm_stream(stream), logits, (long)ld, (long)rows,    \
                       (int)K, targets, (int)pad_id, grad_scale, write_grad ? 1 : 0, loss_rows, logprobs, (long)ldp, \
                       argmax, row_mask, (int)masked_class, labels)
    if (K <= 64) NM_LR(1);
    else if (K <= 128) NM_LR(2);
    else if (K <= 256) NM_LR(4);
    else if (K <= 512) NM_LR(8);
    else NM_LR(16);
#undef NM_LR
    NM_LAUNCH_CHECK("nm_label_rows");
}

int nm_label_rows_from_stats(void* stream, const float* logits, int64_t ld, int64_t rows, int64_t K,
                             const int32_t* targets, int32_t pad_id, const float* rmax, const float* rlse,
                             float* loss_rows, float* weights, const int32_t* argmax, const float* row_mask,
                             int32_t masked_class, int32_t* labels) {
    NM_REQUIRE(K >= 1, "nm_label_rows_from_stats: K = %lld classes, at least 1 is needed", (long long)K);
    NM_REQUIRE(rows >= 0 && rows < (1ll << 31) - 256, "nm_label_rows_from_stats: bad row count %lld", (long long)rows);
    NM_REQUIRE(ld >= K, "nm_label_rows_from_stats: ld %lld below K %lld", (long long)ld, (long long)K);
    NM_REQUIRE(loss_rows == nullptr || targets == nullptr || (logits != nullptr && rmax != nullptr && rlse != nullptr),
               "nm_label_rows_from_stats: loss_rows without logits, rmax or rlse");
    NM_REQUIRE(labels == nullptr || (row_mask != nullptr && argmax != nullptr),
               "nm_label_rows_from_stats: labels without row_mask or argmax");
    if (rows == 0) return NM_OK;
    hipLaunchKernelGGL(label_from_stats_kernel, dim3((unsigned)nm_cdiv(rows, 256)), dim3(256), 0, nm_stream(stream),
                       logits, (long)ld, (long)rows, (long)K, targets, (int)pad_id, rmax, rlse, loss_rows, weights, argmax,
                       row_mask, (int)masked_class, labels);
    NM_LAUNCH_CHECK("nm_label_rows_from_stats");
}

}  // extern "C"
