// The REINFORCE reward over a vocabulary of subword pieces (include/nmhip_subword.h): the evaluators' sentence GLEU /
// BLEU of trainers/rl_trainer.py after its join of BPE pieces, on piece indices, so that a BPE model's training step
// reads nothing back for its rewards either.
//
//   joined_score_kernel   one wavefront per sentence, no atomics.  Per column: the token ids are staged in LDS and the
//                         cut (the first token whose table row carries the cut flag, or whose id is outside the table)
//                         is a 64-wide minimum.  A kept token ends a word unless it is a continuation piece with a kept
//                         token behind it.  A word is the triple (bytes, hash mod M1, hash mod M2), and the hash is
//                         composable -- H(s + t) = H(s) * P^len(t) + H(t) -- so a word's key is the product of its
//                         pieces' table elements (hash, power, length) under an associative composition, and the keys
//                         of all words come out of a SEGMENTED SCAN in registers: 64 positions at a time, six
//                         shuffle steps, the open word at a chunk's end carried into the next chunk.  The alternative,
//                         one lane per word walking its pieces, costs one dependent table read per piece on the lane
//                         with the longest word while the others idle; the scan's cost depends on the column's length
//                         alone, and at a training step's T of 50 it is ONE chunk.  The lanes that hold a word's last
//                         piece write its key to the word's index (a ballot and a population count), which compacts
//                         the keys in LDS; three fillers follow them, different for the two columns and with a
//                         negative length no real word has.  Then, as eval_score_kernel (nm_rl.hip): the lanes run over
//                         the reference's start positions and walk the hypothesis -- a broadcast read -- and the
//                         longest common prefix, capped at 4, answers all orders; integer counts, 64-wide sums, lane 0
//                         finishes in double (nm_score.h) and rounds once.
#include "nm_common.h"
#include "nm_score.h"
#include "../../include/nmhip_subword.h"

namespace {

constexpr int JOIN_MAX_TOKENS = 8192;        // T_ref + T_hyp: 12 * (8192 + 6) + 4 * 8191 bytes of LDS, 128.06 KiB
constexpr int JOIN_PAD = 3;                  // a window of four that starts at the last word stays inside
constexpr int JOIN_ROW = 12;                 // int32 per table row: stem[5], whole[5], flags, 0
constexpr int JOIN_FLAGS = 10, JOIN_CONTINUES = 1, JOIN_CUTS = 2;
constexpr int JOIN_FILL_REF = -1, JOIN_FILL_HYP = -2;        // lengths no word has
constexpr unsigned long long JOIN_M1 = 2147483647ull, JOIN_M2 = 2147483629ull;      // 2^31 - 1, 2^31 - 19: primes

// (hash mod M1, hash mod M2, P1^len mod M1, P2^len mod M2, len) of a piece, of a run of pieces, of a word
struct JoinElem {
    unsigned h1, h2, p1, p2;
    int len;
};

__device__ __forceinline__ JoinElem join_identity() { return JoinElem{0u, 0u, 1u, 1u, 0}; }

// `a` followed by `b`.  Every factor is below 2^31: a product is below 2^62 and the sum below 2^63.
__device__ __forceinline__ JoinElem join_compose(const JoinElem& a, const JoinElem& b) {
    JoinElem c;
    c.h1 = (unsigned)(((unsigned long long)a.h1 * b.p1 + b.h1) % JOIN_M1);
    c.h2 = (unsigned)(((unsigned long long)a.h2 * b.p2 + b.h2) % JOIN_M2);
    c.p1 = (unsigned)(((unsigned long long)a.p1 * b.p1) % JOIN_M1);
    c.p2 = (unsigned)(((unsigned long long)a.p2 * b.p2) % JOIN_M2);
    c.len = a.len + b.len;
    return c;
}

__device__ __forceinline__ JoinElem join_shfl_up(const JoinElem& v, int off) {
    JoinElem r;
    r.h1 = __shfl_up(v.h1, off, 64);
    r.h2 = __shfl_up(v.h2, off, 64);
    r.p1 = __shfl_up(v.p1, off, 64);
    r.p2 = __shfl_up(v.p2, off, 64);
    r.len = __shfl_up(v.len, off, 64);
    return r;
}

__device__ __forceinline__ JoinElem join_shfl(const JoinElem& v, int from) {
    JoinElem r;
    r.h1 = __shfl(v.h1, from, 64);
    r.h2 = __shfl(v.h2, from, 64);
    r.p1 = __shfl(v.p1, from, 64);
    r.p2 = __shfl(v.p2, from, 64);
    r.len = __shfl(v.len, from, 64);
    return r;
}

__device__ __forceinline__ int join_wave_min(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ int join_wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Column `b` of `src` to the keys of its joined words: kh[w] = hash mod M1 << 31 | hash mod M2, kl[w] = bytes, for
// w < the returned number of words (an empty column is the one word of no bytes), and JOIN_PAD fillers behind them.
// `tok` [T] is scratch.  Every loop bound is the same in all lanes: the shuffles and ballots run with 64 lanes.
__device__ __forceinline__ int join_stage(int32_t* tok, unsigned long long* kh, int32_t* kl,
                                          const int32_t* __restrict__ src, long stride, int T, long b,
                                          const int32_t* __restrict__ table, int V, int filler, int lane) {
    int cut = T;
    for (int i = lane; i < T; i += 64) {
        const int32_t t = src[(long)i * stride + b];
        tok[i] = t;
        // (an id outside the table cuts: the row is not read)
        const bool stops = t < 0 || t >= V || (table[(long)t * JOIN_ROW + JOIN_FLAGS] & JOIN_CUTS) != 0;
        if (stops) cut = min(cut, i);
    }
    cut = join_wave_min(cut);
    __syncthreads();

    int words = 0;
    JoinElem carry = join_identity();                 // the pieces of a word that began in an earlier chunk
    for (int base = 0; base < cut; base += 64) {
        const int i = base + lane;
        JoinElem cur = join_identity();
        bool ends = false;
        if (i < cut) {
            const int32_t* row = table + (long)tok[i] * JOIN_ROW;          // 0 <= tok[i] < V in front of the cut
            ends = (row[JOIN_FLAGS] & JOIN_CONTINUES) == 0 || i == cut - 1;
            const int32_t* e = row + (ends ? 5 : 0);                       // the whole text ends a word, the stem goes on
            cur = JoinElem{(unsigned)e[0], (unsigned)e[1], (unsigned)e[2], (unsigned)e[3], e[4]};
        }
        const unsigned long long end_mask = __ballot(ends);
        // a segment begins behind every word's end; lane 0 takes the carry in and begins one
        bool begins = lane == 0 || ((end_mask >> (lane - 1)) & 1ull) != 0;
        if (lane == 0) cur = join_compose(carry, cur);
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const JoinElem left = join_shfl_up(cur, off);
            const int left_begins = __shfl_up((int)begins, off, 64);
            if (lane >= off && !begins) {
                cur = join_compose(left, cur);
                begins = left_begins != 0;
            }
        }
        if (ends) {
            const int w = words + __popcll(end_mask & ((1ull << lane) - 1ull));
            kh[w] = ((unsigned long long)cur.h1 << 31) | (unsigned long long)cur.h2;
            kl[w] = cur.len;
        }
        words += __popcll(end_mask);
        carry = join_shfl(cur, 63);
        if ((end_mask >> 63) & 1ull) carry = join_identity();
    }
    if (cut == 0) {                                   // "".split(" ") == [""]
        if (lane == 0) {
            kh[0] = 0ull;
            kl[0] = 0;
        }
        words = 1;
    }
    if (lane < JOIN_PAD) {
        kh[words + lane] = 0ull;
        kl[words + lane] = filler;
    }
    __syncthreads();
    return words;
}

__global__ __launch_bounds__(64) void joined_score_kernel(
    int kind, int order, const int32_t* __restrict__ ref, long ref_stride, int Tr, const int32_t* __restrict__ hyp,
    long hyp_stride, int Th, const int32_t* __restrict__ table, int V, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long join_lds[];
    unsigned long long* hr = join_lds;                                   // [Tr + JOIN_PAD]
    unsigned long long* hh = hr + Tr + JOIN_PAD;                         // [Th + JOIN_PAD]
    int32_t* lr = reinterpret_cast<int32_t*>(hh + Th + JOIN_PAD);        // [Tr + JOIN_PAD]
    int32_t* lh = lr + Tr + JOIN_PAD;                                    // [Th + JOIN_PAD]
    int32_t* tok = lh + Th + JOIN_PAD;                                   // [max(Tr, Th)]
    const int lane = threadIdx.x;
    const long b = blockIdx.x;
    const int Lr = join_stage(tok, hr, lr, ref, ref_stride, Tr, b, table, V, JOIN_FILL_REF, lane);
    const int Lh = join_stage(tok, hh, lh, hyp, hyp_stride, Th, b, table, V, JOIN_FILL_HYP, lane);

    // tp[k] (order k + 1): reference windows that equal some hypothesis window.  A common prefix never runs into a
    // filler (their lengths differ between the columns and from every word's), so it is as long as both windows are
    // inside their sentences.
    int tp[4] = {0, 0, 0, 0};
    for (int j = lane; j < Lr; j += 64) {
        const unsigned long long a0 = hr[j], a1 = hr[j + 1], a2 = hr[j + 2], a3 = hr[j + 3];
        const int n0 = lr[j], n1 = lr[j + 1], n2 = lr[j + 2], n3 = lr[j + 3];
        int best = 0;
        for (int i = 0; i < Lh; ++i) {
            const int len = (hh[i] != a0 || lh[i] != n0) ? 0
                          : (hh[i + 1] != a1 || lh[i + 1] != n1) ? 1
                          : (hh[i + 2] != a2 || lh[i + 2] != n2) ? 2
                          : (hh[i + 3] != a3 || lh[i + 3] != n3) ? 3 : 4;
            best = max(best, len);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) tp[k] += best > k ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) tp[k] = join_wave_sum(tp[k]);
    if (lane != 0) return;
    out[b] = (float)nm_eval_finish(kind, order, tp, Lr, Lh);
}

}  // namespace

extern "C" {

int64_t nm_eval_joined_sentence_score_max_tokens(void) { return JOIN_MAX_TOKENS; }

int nm_eval_joined_sentence_score(void* stream, int kind, int order, const int32_t* ref, int64_t ref_stride,
                                  int64_t T_ref, const int32_t* hyp, int64_t hyp_stride, int64_t T_hyp, int64_t B,
                                  const int32_t* table, int64_t table_rows, int64_t V, float* out) {
    NM_REQUIRE(kind == 0 || kind == 1, "nm_eval_joined_sentence_score: kind %d (0 BLEU, 1 GLEU)", kind);
    NM_REQUIRE(order >= 1 && order <= 4, "nm_eval_joined_sentence_score: order %d outside 1..4", order);
    NM_REQUIRE(B >= 0 && B < (1ll << 31) && T_ref >= 1 && T_hyp >= 1,
               "nm_eval_joined_sentence_score: bad sizes B %lld, T_ref %lld, T_hyp %lld", (long long)B, (long long)T_ref,
               (long long)T_hyp);
    NM_REQUIRE(T_ref <= JOIN_MAX_TOKENS && T_hyp <= JOIN_MAX_TOKENS && T_ref + T_hyp <= JOIN_MAX_TOKENS,
               "nm_eval_joined_sentence_score: T_ref %lld + T_hyp %lld tokens above the %d the LDS staging holds",
               (long long)T_ref, (long long)T_hyp, JOIN_MAX_TOKENS);
    NM_REQUIRE(ref_stride >= B && hyp_stride >= B, "nm_eval_joined_sentence_score: row strides %lld, %lld below B %lld",
               (long long)ref_stride, (long long)hyp_stride, (long long)B);
    NM_REQUIRE(ref_stride < (1ll << 31) / T_ref && hyp_stride < (1ll << 31) / T_hyp,
               "nm_eval_joined_sentence_score: a token array spans more than 2^31 - 1 elements");
    NM_REQUIRE(V >= 1 && V < (1ll << 31), "nm_eval_joined_sentence_score: vocabulary size %lld", (long long)V);
    NM_REQUIRE(table_rows >= V, "nm_eval_joined_sentence_score: a table of %lld rows for a vocabulary of %lld",
               (long long)table_rows, (long long)V);
    if (B == 0) return NM_OK;
    NM_REQUIRE(ref != nullptr && hyp != nullptr && table != nullptr && out != nullptr,
               "nm_eval_joined_sentence_score: null pointer");
    const int64_t longer = T_ref > T_hyp ? T_ref : T_hyp;
    const size_t lds = (size_t)(T_ref + T_hyp + 2 * JOIN_PAD) * (sizeof(unsigned long long) + sizeof(int32_t)) +
                       (size_t)longer * sizeof(int32_t);
    if (lds > 64 * 1024) {                 // beyond the default limit of a launch; the CU has 160 KiB
        hipError_t e = hipFuncSetAttribute((const void*)joined_score_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)lds);
        if (e != hipSuccess)
            NM_FAIL(NM_ERR_HIP, "nm_eval_joined_sentence_score: %zu bytes of LDS refused: %s", lds, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(joined_score_kernel, dim3((unsigned)B), dim3(64), lds, nm_stream(stream), kind, order, ref,
                       (long)ref_stride, (int)T_ref, hyp, (long)hyp_stride, (int)T_hyp, table, (int)V, out);
    NM_LAUNCH_CHECK("nm_eval_joined_sentence_score");
}

}  // extern "C"
