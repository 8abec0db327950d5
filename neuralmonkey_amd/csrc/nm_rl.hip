// REINFORCE training with sentence-level feedback (include/nmhip_rl.h): the evaluators' sentence GLEU / BLEU of
// trainers/rl_trainer.py on token indices, and the sample-space arithmetic that turns rewards, sentence
// log-probabilities and the running-average baseline into the row weights and scalars of nm_xent -- so that a
// training step reads nothing back after its sampling loops.
//
//   eval_score_kernel          one wavefront per sentence.  Both token columns are staged in LDS, cut at their first
//                              </s> or <pad>; what lies behind the cut (and three tokens behind each array) holds a
//                              filler that is different for the two columns and negative, so a window that reaches
//                              it equals no window of the other column and needs no bounds of its own.  The lanes run
//                              over the REFERENCE's start positions (the count is "reference windows that occur in the
//                              hypothesis") and walk the hypothesis serially -- every lane reads the same LDS words, a
//                              broadcast; the longest common prefix, capped at 4, answers all orders at once.  Integer
//                              counts, 64-wide shuffles, no atomics; lane 0 finishes in double (nm_score.h) and rounds once.
//   rl_sample_weights_kernel   one workgroup: the sum of the rewards (float32, eight interleaved partial sums on one
//                              lane) and the baseline's state, one thread per sentence for the softmax over the
//                              sample axis, then all threads spread the coefficients over the time axis.
#include "nm_common.h"
#include "nm_score.h"
#include "../../include/nmhip_rl.h"

namespace {

constexpr int EVAL_MAX_TOKENS = 8192;        // T_ref + T_hyp: 32 KiB of LDS (+ 24 bytes of filler)
constexpr int EVAL_PAD = 3;                  // a window of four that starts at the last token stays inside
constexpr int EVAL_EMPTY = -1;               // the one word of an empty sentence
constexpr int EVAL_FILL_REF = -2, EVAL_FILL_HYP = -3;
constexpr int RL_THREADS = 1024;
constexpr int RL_MAX_SAMPLES = 64;

struct RlSteps {
    int32_t n[RL_MAX_SAMPLES];
};

__device__ __forceinline__ int eval_wave_min(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ int eval_wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Stage column `b` of `src` into s[0 .. T + EVAL_PAD), cut it at the first end_id or pad_id and return its length in
// words (an empty column is the one word EVAL_EMPTY).
__device__ __forceinline__ int eval_stage(int32_t* s, const int32_t* __restrict__ src, long stride, int T, long b,
                                          int end_id, int pad_id, int filler, int lane) {
    int cut = T;
    for (int i = lane; i < T + EVAL_PAD; i += 64) {
        const int32_t tok = i < T ? src[(long)i * stride + b] : filler;
        s[i] = tok;
        if (i < T && (tok == end_id || tok == pad_id)) cut = min(cut, i);
    }
    cut = eval_wave_min(cut);
    __syncthreads();
    for (int i = cut + lane; i < T; i += 64) s[i] = filler;
    if (cut == 0) {
        if (lane == 0) s[0] = EVAL_EMPTY;
        cut = 1;
    }
    __syncthreads();
    return cut;
}

__global__ __launch_bounds__(64) void eval_score_kernel(
    int kind, int order, const int32_t* __restrict__ ref, long ref_stride, int Tr, const int32_t* __restrict__ hyp,
    long hyp_stride, int Th, int end_id, int pad_id, float* __restrict__ out) {
    extern __shared__ int32_t eval_lds[];
    int32_t* sr = eval_lds;                            // [Tr + EVAL_PAD]
    int32_t* sh = eval_lds + Tr + EVAL_PAD;            // [Th + EVAL_PAD]
    const int lane = threadIdx.x;
    const long b = blockIdx.x;
    const int Lr = eval_stage(sr, ref, ref_stride, Tr, b, end_id, pad_id, EVAL_FILL_REF, lane);
    const int Lh = eval_stage(sh, hyp, hyp_stride, Th, b, end_id, pad_id, EVAL_FILL_HYP, lane);

    // tp[k] (order k + 1): reference windows that equal some hypothesis window.  A common prefix never runs into a
    // filler (they differ between the columns), so it is as long as both windows are inside their sentences.
    int tp[4] = {0, 0, 0, 0};
    for (int j = lane; j < Lr; j += 64) {
        const int r0 = sr[j], r1 = sr[j + 1], r2 = sr[j + 2], r3 = sr[j + 3];
        int best = 0;
        for (int i = 0; i < Lh; ++i) {
            const int len = sh[i] != r0 ? 0 : sh[i + 1] != r1 ? 1 : sh[i + 2] != r2 ? 2 : sh[i + 3] != r3 ? 3 : 4;
            best = max(best, len);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) tp[k] += best > k ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) tp[k] = eval_wave_sum(tp[k]);
    if (lane != 0) return;

    out[b] = (float)nm_eval_finish(kind, order, tp, Lr, Lh);
}

// The sum of every thread's `v` in a fixed order, handed to every thread.
__device__ __forceinline__ double rl_block_sum(double v, double* partial) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();                                   // (partial may still be read from the sum before)
    if ((threadIdx.x & 63) == 0) partial[threadIdx.x >> 6] = v;
    __syncthreads();
    double total = 0.0;
    for (int w = 0; w < RL_THREADS / 64; ++w) total += partial[w];
    return total;
}

__global__ __launch_bounds__(RL_THREADS) void rl_sample_weights_kernel(
    const float* __restrict__ rewards, const float* __restrict__ logprobs, RlSteps steps, int S, int T, int B,
    int subtract_baseline, int normalize, float alpha, float weight, float* __restrict__ reward_counter,
    float* __restrict__ reward_sum, float* weights, float* __restrict__ grad_scale,
    float* __restrict__ loss, float* __restrict__ baseline_out) {
    __shared__ double partial[RL_THREADS / 64];
    __shared__ float base_shared;
    const int tid = threadIdx.x;

    if (tid == 0) {
        float base = 0.0f;
        if (subtract_baseline) {
            // tf.reduce_sum of float32 rewards accumulates in float32, and so does this, on one lane: eight interleaved
            // partial sums (eight independent chains of adds), combined pairwise, then the tail -- the order NumPy's
            // float32 sum takes for up to 128 numbers, so a host restatement of a step with S * B <= 128 is bit-equal
            const int n = S * B;
            float total = 0.0f;
            if (n < 8) {
                for (int i = 0; i < n; ++i) total += rewards[i];
            } else {
                float r[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) r[j] = rewards[j];
                int i = 8;
                for (; i < n - n % 8; i += 8) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) r[j] += rewards[i + j];
                }
                total = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
                for (; i < n; ++i) total += rewards[i];
            }
            const float counter = reward_counter[0] + (float)(S * B);
            const float sum = reward_sum[0] + total;
            reward_counter[0] = counter;
            reward_sum[0] = sum;
            base = sum / fmaxf(counter, 1.0f);
        }
        base_shared = base;
        baseline_out[0] = base;
        grad_scale[0] = weight;
    }
    __syncthreads();
    const double base = (double)base_shared;

    // one thread per sentence: the coefficients -d loss / d sent_logprob go to the weights' rows of t = 0 (every loop
    // has one), the sentence's share of the loss to the sum
    double loss_mine = 0.0;
    for (int b = tid; b < B; b += RL_THREADS) {
        if (normalize) {
            double top = -INFINITY;
            for (int s = 0; s < S; ++s) top = fmax(top, (double)alpha * (double)logprobs[s * B + b]);
            double denom = 0.0, expected = 0.0;
            for (int s = 0; s < S; ++s) {
                const double e = exp((double)alpha * (double)logprobs[s * B + b] - top);
                denom += e;
                expected += -((double)rewards[s * B + b] - base) * e;
            }
            expected /= denom;
            for (int s = 0; s < S; ++s) {
                const double p = exp((double)alpha * (double)logprobs[s * B + b] - top) / denom;
                const double a = -((double)rewards[s * B + b] - base);
                weights[(long)s * T * B + b] = (float)(-(double)alpha * p * (a - expected) / (double)B);
            }
            loss_mine += expected;
        } else {
            for (int s = 0; s < S; ++s) {
                const double a = -((double)rewards[s * B + b] - base);
                weights[(long)s * T * B + b] = (float)(-a / (double)B);
                if (logprobs != nullptr) loss_mine += a * (double)logprobs[s * B + b];
            }
        }
    }
    const double loss_total = rl_block_sum(loss_mine, partial);
    if (tid == 0 && loss != nullptr && (normalize || logprobs != nullptr)) loss[0] = (float)(loss_total / (double)B);
    __threadfence_block();
    __syncthreads();
    // ... and over the time axis: row t of sample s repeats row 0 while t < steps[s]
    const int per_sample = T * B;
    for (int i = tid; i < S * per_sample; i += RL_THREADS) {
        const int s = i / per_sample, rest = i - s * per_sample;
        const int t = rest / B, b = rest - t * B;
        if (t == 0) continue;
        weights[i] = t < steps.n[s] ? weights[(long)s * per_sample + b] : 0.0f;
    }
}

}  // namespace

extern "C" {

int64_t nm_eval_sentence_score_max_tokens(void) { return EVAL_MAX_TOKENS; }

int64_t nm_reinforce_sample_weights_max_samples(void) { return RL_MAX_SAMPLES; }

int nm_eval_sentence_score(void* stream, int kind, int order, const int32_t* ref, int64_t ref_stride, int64_t T_ref,
                           const int32_t* hyp, int64_t hyp_stride, int64_t T_hyp, int64_t B, int32_t end_id,
                           int32_t pad_id, float* out) {
    NM_REQUIRE(kind == 0 || kind == 1, "nm_eval_sentence_score: kind %d (0 BLEU, 1 GLEU)", kind);
    NM_REQUIRE(order >= 1 && order <= 4, "nm_eval_sentence_score: order %d outside 1..4", order);
    NM_REQUIRE(B >= 0 && B < (1ll << 31) && T_ref >= 1 && T_hyp >= 1,
               "nm_eval_sentence_score: bad sizes B %lld, T_ref %lld, T_hyp %lld", (long long)B, (long long)T_ref,
               (long long)T_hyp);
    NM_REQUIRE(T_ref <= EVAL_MAX_TOKENS && T_hyp <= EVAL_MAX_TOKENS && T_ref + T_hyp <= EVAL_MAX_TOKENS,
               "nm_eval_sentence_score: T_ref %lld + T_hyp %lld tokens above the %d the LDS staging holds",
               (long long)T_ref, (long long)T_hyp, EVAL_MAX_TOKENS);
    NM_REQUIRE(ref_stride >= B && hyp_stride >= B, "nm_eval_sentence_score: row strides %lld, %lld below B %lld",
               (long long)ref_stride, (long long)hyp_stride, (long long)B);
    NM_REQUIRE(ref_stride < (1ll << 31) / T_ref && hyp_stride < (1ll << 31) / T_hyp,
               "nm_eval_sentence_score: a token array spans more than 2^31 - 1 elements");
    NM_REQUIRE(end_id >= 0 && pad_id >= 0 && end_id != pad_id, "nm_eval_sentence_score: end_id %d, pad_id %d",
               (int)end_id, (int)pad_id);
    if (B == 0) return NM_OK;
    NM_REQUIRE(ref != nullptr && hyp != nullptr && out != nullptr, "nm_eval_sentence_score: null pointer");
    const size_t lds = (size_t)(T_ref + T_hyp + 2 * EVAL_PAD) * sizeof(int32_t);
    hipLaunchKernelGGL(eval_score_kernel, dim3((unsigned)B), dim3(64), lds, nm_stream(stream), kind, order, ref,
                       (long)ref_stride, (int)T_ref, hyp, (long)hyp_stride, (int)T_hyp, (int)end_id, (int)pad_id, out);
    NM_LAUNCH_CHECK("nm_eval_sentence_score");
}

int nm_reinforce_sample_weights(void* stream, const float* rewards, const float* sent_logprobs, const int32_t* steps,
                                int64_t S, int64_t T, int64_t B, int subtract_baseline, int normalize, float alpha,
                                float weight, float* reward_counter, float* reward_sum, float* weights,
                                float* grad_scale, float* loss, float* baseline) {
    NM_REQUIRE(S >= 1 && S <= RL_MAX_SAMPLES && T >= 1 && B >= 1,
               "nm_reinforce_sample_weights: bad sizes S %lld (1..%d), T %lld, B %lld", (long long)S, RL_MAX_SAMPLES,
               (long long)T, (long long)B);
    NM_REQUIRE(T < (1ll << 31) / B && S < (1ll << 31) / (T * B), "nm_reinforce_sample_weights: S * T * B beyond 2^31 - 1");
    NM_REQUIRE(rewards != nullptr && steps != nullptr && weights != nullptr && grad_scale != nullptr &&
               baseline != nullptr, "nm_reinforce_sample_weights: null pointer");
    NM_REQUIRE(!normalize || sent_logprobs != nullptr, "nm_reinforce_sample_weights: normalize without sent_logprobs");
    NM_REQUIRE(!subtract_baseline || (reward_counter != nullptr && reward_sum != nullptr),
               "nm_reinforce_sample_weights: subtract_baseline without its state");
    RlSteps packed;
    memset(&packed, 0, sizeof(packed));
    for (int64_t s = 0; s < S; ++s) {
        NM_REQUIRE(steps[s] >= 1 && steps[s] <= T, "nm_reinforce_sample_weights: loop length %d of sample %lld outside 1..%lld",
                   (int)steps[s], (long long)s, (long long)T);
        packed.n[s] = steps[s];
    }
    hipLaunchKernelGGL(rl_sample_weights_kernel, dim3(1), dim3(RL_THREADS), 0, nm_stream(stream), rewards, sent_logprobs,
                       packed, (int)S, (int)T, (int)B, subtract_baseline, normalize, alpha, weight, reward_counter,
                       reward_sum, weights, grad_scale, loss, baseline);
    NM_LAUNCH_CHECK("nm_reinforce_sample_weights");
}

}  // extern "C"
