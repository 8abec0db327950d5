// The final arithmetic of the evaluators' sentence GLEU / BLEU, shared by eval_score_kernel (nm_rl.hip, words are token
// indices) and joined_score_kernel (nm_subword.hip, words are joined pieces): from the integer counts to one double,
// which the caller rounds once to float.  One lane calls it.
#pragma once
#include <hip/hip_runtime.h>

// tp[k] (order k + 1): reference windows that equal some hypothesis window; Lr, Lh >= 1: the lengths in words.
__device__ __forceinline__ double nm_eval_finish(int kind, int order, const int (&tp)[4], int Lr, int Lh) {
    double score;
    if (kind == 1) {
        long sum_tp = 0, sum_gen = 0, sum_tgt = 0;           // |hyp|, |ref| >= 1: neither total is 0
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < order) {
                sum_tp += tp[k];
                sum_gen += max(0, Lh - k);
                sum_tgt += max(0, Lr - k);
            }
        score = fmin((double)sum_tp / (double)sum_tgt, (double)sum_tp / (double)sum_gen);
    } else {
        const double weight = 1.0 / (double)order;
        double log_bleu = 0.0, smooth = 1.0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < order) {
                const int gen = max(0, Lh - k);
                double prec = gen == 0 ? 1.0 : (double)tp[k] / (double)gen;
                if (prec == 0.0) {
                    smooth *= 2.0;
                    prec = 1.0 / (smooth * (double)gen);
                }
                log_bleu += weight * log(prec);
            }
        log_bleu += fmin(1.0 - (double)Lr / (double)Lh, 0.0);
        score = 100.0 * exp(log_bleu);
    }
    return score;
}
