// Sentence-level rewards of self-critical training (include/nmhip_reward.h): sentence_bleu / sentence_gleu of
// trainers/self_critical_objective.py on token indices, and the row weights and scalars that turn nm_xent over the
// runtime logits into the REINFORCE loss -- so that a training step reads nothing back after its decoding loop.
//
//   reward_sentence_kernel   one wavefront per sentence.  Both token columns are staged in LDS (three padding tokens
//                            behind each, so that a window of four never reads past its array); the lanes run over the
//                            hypothesis' start positions (several per lane above 64 tokens) and walk the comparison
//                            positions serially -- every lane reads the same LDS words, a broadcast.  One pass serves
//                            the four orders: the match length of a window pair, capped at 4, extends the equality of
//                            the (n-1)-grams by one token.  Integer counts, 64-wide shuffles, no atomics; lane 0
//                            finishes in double and rounds once.  (The pass and the score live in nm_ngram.h,
//                            which nm_mbr.hip shares.)
//   reinforce_weights_kernel one workgroup: the weights, an integer count of the mask and the two scalars.
#include "nm_common.h"
#include "nm_ngram.h"
#include "../../include/nmhip_reward.h"

namespace {

constexpr int RW_THREADS = 1024;

__global__ __launch_bounds__(64) void reward_sentence_kernel(
    int kind, const int32_t* __restrict__ ref, long ref_stride, int Tr, const int32_t* __restrict__ hyp,
    long hyp_stride, int Th, int end_id, float* __restrict__ out) {
    extern __shared__ int32_t reward_lds[];
    int32_t* sr = reward_lds;                          // [Tr + REWARD_PAD]
    int32_t* sh = reward_lds + Tr + REWARD_PAD;        // [Th + REWARD_PAD]
    const int lane = threadIdx.x;
    const long b = blockIdx.x;
    for (int i = lane; i < Tr + REWARD_PAD; i += 64) sr[i] = i < Tr ? ref[(long)i * ref_stride + b] : 0;
    for (int i = lane; i < Th + REWARD_PAD; i += 64) sh[i] = i < Th ? hyp[(long)i * hyp_stride + b] : 0;
    __syncthreads();

    int er[4], eh[4];
    reward_ends(sr, Tr, end_id, lane, er);
    reward_ends(sh, Th, end_id, lane, eh);

    int matched[4];
    reward_matched(sh, Th, eh, sr, Tr, er, lane, matched);
    if (lane != 0) return;
    out[b] = (float)reward_score(kind, matched, eh, er);
}

__global__ __launch_bounds__(RW_THREADS) void reinforce_weights_kernel(
    const float* __restrict__ reward, const float* __restrict__ baseline, const int32_t* __restrict__ mask, int n, int B,
    float weight, float* __restrict__ weights, float* __restrict__ grad_scale, float* __restrict__ inv_count) {
    __shared__ int partial[RW_THREADS / 64];
    int count = 0;
    for (int i = threadIdx.x; i < n; i += RW_THREADS) {
        const int m = mask[i];
        const int b = i % B;
        weights[i] = -(reward[b] - baseline[b]) * (float)m;
        count += m;
    }
    count = reward_wave_sum(count);
    if ((threadIdx.x & 63) == 0) partial[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < RW_THREADS / 64; ++w) total += partial[w];
        grad_scale[0] = total != 0 ? weight / (float)total : 0.0f;
        inv_count[0] = total != 0 ? 1.0f / (float)total : 0.0f;
    }
}

}  // namespace

extern "C" {

int64_t nm_sentence_reward_max_tokens(void) { return REWARD_MAX_TOKENS; }

int nm_sentence_reward(void* stream, int kind, const int32_t* ref, int64_t ref_stride, int64_t T_ref,
                       const int32_t* hyp, int64_t hyp_stride, int64_t T_hyp, int64_t B, int32_t end_id, float* out) {
    NM_REQUIRE(kind == 0 || kind == 1, "nm_sentence_reward: kind %d (0 BLEU, 1 GLEU)", kind);
    NM_REQUIRE(B >= 0 && B < (1ll << 31) && T_ref >= 1 && T_hyp >= 1,
               "nm_sentence_reward: bad sizes B %lld, T_ref %lld, T_hyp %lld", (long long)B, (long long)T_ref,
               (long long)T_hyp);
    NM_REQUIRE(T_ref <= REWARD_MAX_TOKENS && T_hyp <= REWARD_MAX_TOKENS && T_ref + T_hyp <= REWARD_MAX_TOKENS,
               "nm_sentence_reward: T_ref %lld + T_hyp %lld tokens above the %d the LDS staging holds",
               (long long)T_ref, (long long)T_hyp, REWARD_MAX_TOKENS);
    NM_REQUIRE(ref_stride >= B && hyp_stride >= B, "nm_sentence_reward: row strides %lld, %lld below B %lld",
               (long long)ref_stride, (long long)hyp_stride, (long long)B);
    NM_REQUIRE(ref_stride < (1ll << 31) / T_ref && hyp_stride < (1ll << 31) / T_hyp,
               "nm_sentence_reward: a token array spans more than 2^31 - 1 elements");
    if (B == 0) return NM_OK;
    NM_REQUIRE(ref != nullptr && hyp != nullptr && out != nullptr, "nm_sentence_reward: null pointer");
    const size_t lds = (size_t)(T_ref + T_hyp + 2 * REWARD_PAD) * sizeof(int32_t);
    hipLaunchKernelGGL(reward_sentence_kernel, dim3((unsigned)B), dim3(64), lds, nm_stream(stream), kind, ref,
                       (long)ref_stride, (int)T_ref, hyp, (long)hyp_stride, (int)T_hyp, (int)end_id, out);
    NM_LAUNCH_CHECK("nm_sentence_reward");
}

int nm_reinforce_weights(void* stream, const float* reward, const float* baseline, const int32_t* mask, int64_t T,
                         int64_t B, float weight, float* weights, float* grad_scale, float* inv_count) {
    NM_REQUIRE(T >= 1 && B >= 1, "nm_reinforce_weights: bad sizes T %lld, B %lld", (long long)T, (long long)B);
    NM_REQUIRE(T < (1ll << 31) / B, "nm_reinforce_weights: T * B beyond 2^31 - 1");
    NM_REQUIRE(reward != nullptr && baseline != nullptr && mask != nullptr && weights != nullptr &&
               grad_scale != nullptr && inv_count != nullptr, "nm_reinforce_weights: null pointer");
    hipLaunchKernelGGL(reinforce_weights_kernel, dim3(1), dim3(RW_THREADS), 0, nm_stream(stream), reward, baseline, mask,
                       (int)(T * B), (int)B, weight, weights, grad_scale, inv_count);
    NM_LAUNCH_CHECK("nm_reinforce_weights");
}

}  // extern "C"
