// The n-gram arithmetic of sentence_bleu / sentence_gleu (trainers/self_critical_objective.py) for one wavefront, shared
// by the rewards of self-critical training (nm_reward.hip) and the pairwise utilities of MBR decoding (nm_mbr.hip):
// the ends e_n, the clipped match counts of the orders 1..4 in one pass, and the score in double.  The rule is stated
// in include/nmhip_reward.h.
#pragma once
#include "nm_common.h"

constexpr int REWARD_MAX_TOKENS = 8192;      // both staged columns together: 32 KiB of LDS (+ 24 bytes of padding)
constexpr int REWARD_PAD = 3;                // a window of four that starts at the last token stays inside

__device__ __forceinline__ int reward_wave_min(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ int reward_wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// e[k] (order n = k + 1): the first index >= k of `s` that holds end_id, or T
__device__ __forceinline__ void reward_ends(const int32_t* s, int T, int end_id, int lane, int e[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) e[k] = T;
    for (int i = lane; i < T; i += 64)
        if (s[i] == end_id) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i >= k) e[k] = min(e[k], i);
        }
#pragma unroll
    for (int k = 0; k < 4; ++k) e[k] = reward_wave_min(e[k]);
}

// matched[k]: the clipped count of the order k + 1, summed over the wavefront.  sh and sr are staged in LDS with
// REWARD_PAD tokens behind each; the lanes run over the hypothesis' start positions below nh and walk the comparison
// positions (below nr in the reference) serially -- every lane reads the same LDS words, a broadcast.  One pass
// serves the four orders: the match length of a window pair, capped at 4, extends the equality of the (n-1)-grams by
// one token.  A padding token may compare equal to a real one; that never counts: a window of order k + 1 at j counts
// only with j + k < e[k] <= T, where all its tokens are real.  nh >= eh[3] and nr >= er[3] lose nothing: no window
// at or behind e[3] counts for any order (e[0] <= e[1] <= e[2] <= e[3]).
__device__ __forceinline__ void reward_matched(const int32_t* sh, int nh, const int eh[4], const int32_t* sr, int nr,
                                               const int er[4], int lane, int matched[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) matched[k] = 0;
    for (int i = lane; i < nh; i += 64) {
        const int h0 = sh[i], h1 = sh[i + 1], h2 = sh[i + 2], h3 = sh[i + 3];
        int before[4] = {0, 0, 0, 0}, inref[4] = {0, 0, 0, 0};
        for (int j = 0; j < i; ++j) {
            const int len = sh[j] != h0 ? 0 : sh[j + 1] != h1 ? 1 : sh[j + 2] != h2 ? 2 : sh[j + 3] != h3 ? 3 : 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) before[k] += (len > k && j + k < eh[k]) ? 1 : 0;
        }
        for (int j = 0; j < nr; ++j) {
            const int len = sr[j] != h0 ? 0 : sr[j + 1] != h1 ? 1 : sr[j + 2] != h2 ? 2 : sr[j + 3] != h3 ? 3 : 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) inref[k] += (len > k && j + k < er[k]) ? 1 : 0;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) matched[k] += (i + k < eh[k] && before[k] < inref[k]) ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) matched[k] = reward_wave_sum(matched[k]);
}

// kind 0 BLEU, kind 1 GLEU from the counts of one (reference, hypothesis) pair; in double, rounded once by the caller
__device__ __forceinline__ double reward_score(int kind, const int matched[4], const int eh[4], const int er[4]) {
    int tot_h[4], tot_r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        tot_h[k] = max(0, eh[k] - k);
        tot_r[k] = max(0, er[k] - k);
    }
    double score = 0.0;
    if (kind == 0) {
        if (tot_h[0] > 0) {
            long long pm = matched[0], pt = tot_h[0];             // at most 8192^4 = 2^52
#pragma unroll
            for (int k = 1; k < 4; ++k) {
                pm *= matched[k] + 1;
                pt *= tot_h[k] + 1;
            }
            const double precision = pow((double)pm / (double)pt, 0.25);
            const double brevity = fmin(1.0, exp(1.0 - (double)er[0] / (double)tot_h[0]));
            score = brevity * precision;
        }
    } else {
        int sm = 0, sth = 0, str = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            sm += matched[k];
            sth += tot_h[k];
            str += tot_r[k];
        }
        if (sth > 0 && str > 0) score = fmin((double)sm / (double)sth, (double)sm / (double)str);
    }
    return score;
}
