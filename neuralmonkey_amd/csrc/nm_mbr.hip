// Minimum Bayes risk decoding over the samples of a sentence (include/nmhip_mbr.h): the pairwise
// sentence_bleu / sentence_gleu utilities of the n samples SamplingDecoder drew, and the choice of the sample with the
// highest expected utility -- so that a decoding run reads back one sentence per input, not n.
//
//   mbr_pairwise_kernel   one wavefront per unordered pair i <= j of one sentence (grid: pairs x sentences).  Both
//                         token columns are staged in LDS with three padding tokens behind each, as in
//                         reward_sentence_kernel; the matching pass and the score are that kernel's (nm_ngram.h), with
//                         the lanes bounded by the columns' ends e_4 instead of T (the <pad> tail costs nothing).  The
//                         clipped count min(count in i, count in j) per n-gram does not depend on which column is the
//                         hypothesis, so ONE pass yields U[i, j] and U[j, i]: lane 0 finishes both directions in
//                         double.  Integer counts, 64-wide shuffles, no atomics.
//   mbr_select_kernel     one wavefront per sentence: lane i sums row i of U in j order in double, a butterfly on
//                         (valid, sum, index) finds the argmax (NaN behind everything, ties to the lowest index), and
//                         the lanes copy the chosen column.
#include "nm_common.h"
#include "nm_ngram.h"
#include "../../include/nmhip_mbr.h"

namespace {

constexpr int MBR_MAX_SAMPLES = 64;          // one lane per sample in mbr_select_kernel

__global__ __launch_bounds__(64) void mbr_pairwise_kernel(int kind, const int32_t* __restrict__ tok, long t_stride,
                                                          int T, long B, int n, int end_id, float* __restrict__ U) {
    extern __shared__ int32_t mbr_lds[];
    int32_t* si = mbr_lds;                             // [T + REWARD_PAD] sample i
    int32_t* sj = mbr_lds + T + REWARD_PAD;            // [T + REWARD_PAD] sample j
    const int lane = threadIdx.x;
    int i = 0, j = blockIdx.x;                         // pair blockIdx.x of the rows (0,0) .. (0,n-1), (1,1) .. (1,n-1), ...
    while (j >= n - i) {
        j -= n - i;
        ++i;
    }
    j += i;
    for (long b = blockIdx.y; b < B; b += gridDim.y) {
        const int32_t* col = tok + b * n;
        for (int t = lane; t < T + REWARD_PAD; t += 64) {
            si[t] = t < T ? col[(long)t * t_stride + i] : 0;
            sj[t] = t < T ? col[(long)t * t_stride + j] : 0;
        }
        __syncthreads();

        int ei[4], ej[4], matched[4];
        reward_ends(si, T, end_id, lane, ei);
        reward_ends(sj, T, end_id, lane, ej);
        reward_matched(si, ei[3], ei, sj, ej[3], ej, lane, matched);
        if (lane == 0) {
            float* u = U + b * n * n;
            u[i * n + j] = (float)reward_score(kind, matched, ei, ej);                 // hypothesis i, reference j
            if (i != j) u[j * n + i] = (float)reward_score(kind, matched, ej, ei);     // hypothesis j, reference i
        }
        __syncthreads();                               // the columns are read to the end before the next are staged
    }
}

__global__ __launch_bounds__(64) void mbr_select_kernel(const float* __restrict__ U, const int32_t* __restrict__ tok,
                                                        long t_stride, int T, long B, int n,
                                                        float* __restrict__ expected, int32_t* __restrict__ best,
                                                        int32_t* __restrict__ chosen) {
    const int lane = threadIdx.x;
    for (long b = blockIdx.x; b < B; b += gridDim.x) {
        double sum = 0.0;
        int valid = 0, idx = lane;
        if (lane < n) {
            const float* row = U + (b * n + lane) * n;
            for (int j = 0; j < n; ++j) sum += (double)row[j];
            expected[b * n + lane] = (float)(sum / (double)n);
            valid = isnan(sum) ? 0 : 1;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {       // every lane ends with the same winner: the order is total
            const double other_sum = __shfl_xor(sum, off, 64);
            const int other_idx = __shfl_xor(idx, off, 64), other_valid = __shfl_xor(valid, off, 64);
            if (other_valid && (!valid || other_sum > sum || (other_sum == sum && other_idx < idx))) {
                sum = other_sum;
                idx = other_idx;
                valid = 1;
            }
        }
        const int win = valid ? idx : 0;
        if (lane == 0) best[b] = win;
        const int32_t* col = tok + b * n + win;
        for (int t = lane; t < T; t += 64) chosen[(long)t * B + b] = col[(long)t * t_stride];
    }
}

// the checks the two entry points share; `what` names the entry point
int mbr_check_sizes(const char* what, int64_t t_stride, int64_t T, int64_t B, int64_t n) {
    NM_REQUIRE(n >= 1 && n <= MBR_MAX_SAMPLES, "%s: n %lld samples outside 1..%d", what, (long long)n, MBR_MAX_SAMPLES);
    NM_REQUIRE(B >= 0 && T >= 1, "%s: bad sizes B %lld, T %lld", what, (long long)B, (long long)T);
    NM_REQUIRE(B < (1ll << 31) / (n * n), "%s: B %lld * n %lld * n beyond 2^31 - 1", what, (long long)B, (long long)n);
    NM_REQUIRE(t_stride >= B * n, "%s: row stride %lld below B * n = %lld", what, (long long)t_stride,
               (long long)(B * n));
    NM_REQUIRE(t_stride < (1ll << 31) / T, "%s: the token array spans more than 2^31 - 1 elements", what);
    return NM_OK;
}

}  // namespace

extern "C" {

int nm_mbr_pairwise(void* stream, int kind, const int32_t* tok, int64_t t_stride, int64_t T, int64_t B, int64_t n,
                    int32_t end_id, float* U) {
    NM_REQUIRE(kind == 0 || kind == 1, "nm_mbr_pairwise: kind %d (0 BLEU, 1 GLEU)", kind);
    if (int rc = mbr_check_sizes("nm_mbr_pairwise", t_stride, T, B, n)) return rc;
    NM_REQUIRE(2 * T <= REWARD_MAX_TOKENS, "nm_mbr_pairwise: 2 * T = %lld tokens above the %d the LDS staging holds",
               (long long)(2 * T), REWARD_MAX_TOKENS);
    NM_REQUIRE(end_id >= 0, "nm_mbr_pairwise: negative end_id %d", (int)end_id);
    if (B == 0) return NM_OK;
    NM_REQUIRE(tok != nullptr && U != nullptr, "nm_mbr_pairwise: null pointer");
    const size_t lds = (size_t)(2 * (T + REWARD_PAD)) * sizeof(int32_t);
    hipLaunchKernelGGL(mbr_pairwise_kernel, dim3((unsigned)(n * (n + 1) / 2), nm_grid_rows(B)), dim3(64), lds,
                       nm_stream(stream), kind, tok, (long)t_stride, (int)T, (long)B, (int)n, (int)end_id, U);
    NM_LAUNCH_CHECK("nm_mbr_pairwise");
}

int nm_mbr_select(void* stream, const float* U, const int32_t* tok, int64_t t_stride, int64_t T, int64_t B, int64_t n,
                  float* expected, int32_t* best, int32_t* chosen) {
    if (int rc = mbr_check_sizes("nm_mbr_select", t_stride, T, B, n)) return rc;
    if (B == 0) return NM_OK;
    NM_REQUIRE(U != nullptr && tok != nullptr && expected != nullptr && best != nullptr && chosen != nullptr,
               "nm_mbr_select: null pointer");
    hipLaunchKernelGGL(mbr_select_kernel, dim3((unsigned)(B < (1 << 20) ? B : (1 << 20))), dim3(64), 0,
                       nm_stream(stream), U, tok, (long)t_stride, (int)T, (long)B, (int)n, expected, best, chosen);
    NM_LAUNCH_CHECK("nm_mbr_select");
}

}  // extern "C"
