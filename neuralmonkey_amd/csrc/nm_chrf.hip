// chrF of sentences (include/nmhip_chrf.h): the character n-gram F-score of a reference and a hypothesis
// column of token indices -- the reward of self-critical training (nm_chrf_reward) and the utility of minimum Bayes risk
// decoding (nm_chrf_pairwise).  The characters come from a device-resident table of the vocabulary; nothing is read
// back.  ONE wavefront owns one pair, and its workgroup is that wavefront:
//
//   expansion  per column.  The lanes read the tokens 64 at a time and find the cut e (end_id or an index outside the
//              table) with a 64-wide minimum.  A second sweep over the tokens below e gives every lane its token's row:
//              the length it contributes (the stem of a glued piece that is not last, else the whole word; one more
//              for the space unless glued, last or dropped), clamped to max_word_chars.  An inclusive wave scan and a
//              carry between chunks place the tokens in the stream.  The copy runs over the CHARACTERS of a chunk, 64
//              at a time: a lane finds the token that holds its character by six steps of bisection over the lanes'
//              scan values (ds_bpermute), then reads chars[] or writes the space.  A 70-character word is two such
//              rounds of the whole wavefront, not 70 steps of one lane.  The stream is uint16 in LDS; five fillers
//              follow it, 0xFFFF behind the reference and 0xFFFE behind the hypothesis.
//   bound      a column of T tokens yields at most T (max_word_chars + 1) characters whatever the table holds, because of
//              the clamp; the launch sizes the LDS by that product, so no table can cause a write outside it.
//   matching   reward_matched of nm_ngram.h for up to six orders.  The lanes run over the start positions i of the
//              SHORTER stream (matched is symmetric, and the work is its length times the other's) and keep the N
//              characters at i in registers.  They walk the positions j < i of their own stream and all j of the other
//              one; every lane reads the same LDS halfword, a broadcast, and a window slides through registers: one
//              LDS read per step.  The equality prefix p_1 >= p_2 >= ... >= p_N of a window pair answers all orders:
//              counts before[k] (equal k-grams earlier in the own stream) and other[k]; the k-gram at i is matched
//              iff before[k] < other[k].  A window that runs past its stream's end holds a filler no other window
//              holds (fillers differ between the streams and from every character), so it never counts and no bound
//              is tested.  No sorting, no hashing: exact for any alphabet.  Integer counts, 64-wide sums.
//   finish     lane 0 (and lane 1 for the other direction of a pair), in double without contraction, rounded once.
#include "nm_common.h"
#include "../../include/nmhip_chrf.h"

namespace {

constexpr int CHRF_MAX_CHARS = 16384;                    // nm_chrf_max_chars(): 32 KiB of uint16
constexpr int CHRF_PAD = NM_CHRF_MAX_ORDER - 1;          // a window of six that starts at the last character stays inside
constexpr int CHRF_MAX_SAMPLES = 64;                     // as nm_mbr_select: one lane per sample there
constexpr int CHRF_MAX_WAVEFRONTS = 1 << 25;             // of one launch: 2^31 threads, which every runtime takes
constexpr unsigned CHRF_FILL_REF = 0xFFFF, CHRF_FILL_HYP = 0xFFFE;

struct ChrfTable {
    const int4* rows;                                    // (offset, stem_len, whole_len, flags)
    const uint16_t* chars;
    int V, max_word;
};

__device__ __forceinline__ int chrf_wave_min(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ int chrf_wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ int chrf_wave_scan(int v, int lane) {          // inclusive
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int below = __shfl_up(v, off, 64);
        v += lane >= off ? below : 0;
    }
    return v;
}

// The characters of the column's sentence into dst, CHRF_PAD fillers behind them; returns their number, at most
// T * (tab.max_word + 1).  Called by all 64 lanes; element t of the column at col[t * stride].
__device__ __forceinline__ int chrf_expand(uint16_t* dst, const int32_t* col, long stride, int T, int end_id,
                                           const ChrfTable& tab, unsigned filler, int lane) {
    int e = T;
    for (int t = lane; t < T; t += 64) {
        const int32_t v = col[(long)t * stride];
        if (v == end_id || v < 0 || v >= tab.V) e = min(e, t);
    }
    e = chrf_wave_min(e);
    int base = 0;                                        // the characters of the chunks before this one
    for (int t0 = 0; t0 < e; t0 += 64) {                 // e is uniform: all lanes take every shuffle below
        const int t = t0 + lane;
        int src = 0, word = 0, own = 0;                  // own = word + the space behind it
        if (t < e) {
            const int4 row = tab.rows[col[(long)t * stride]];
            const bool last = t + 1 == e, glued = (row.w & NM_CHRF_GLUE) != 0 && !last;
            src = row.x;
            word = min(max(glued ? row.y : row.z, 0), tab.max_word);
            own = word + ((glued || last || (row.w & NM_CHRF_SPACE_DROPPED) != 0) ? 0 : 1);
        }
        const int upto = chrf_wave_scan(own, lane);      // the chunk's characters up to and with this lane's token
        const int total = __shfl(upto, 63, 64);
        for (int c0 = 0; c0 < total; c0 += 64) {
            const int c = c0 + lane;
            int owner = 0;                               // the lanes whose tokens end at or before c: 63 at the most,
#pragma unroll                                           // reached where c >= total, on a lane that stores nothing
            for (int step = 32; step > 0; step >>= 1)
                owner += __shfl(upto, owner + step - 1, 64) <= c ? step : 0;
            const int first = __shfl(upto - own, owner, 64), from = __shfl(src, owner, 64);
            const int length = __shfl(word, owner, 64), k = c - first;
            if (c < total) dst[base + c] = k < length ? tab.chars[(long)from + k] : (uint16_t)NM_CHRF_SPACE_ID;
        }
        base += total;
    }
    if (lane < CHRF_PAD) dst[base + lane] = (uint16_t)filler;
    return base;
}

// acc[k] += the number of positions j < count of s whose k + 1 characters equal h[0..k]
template <int N>
__device__ __forceinline__ void chrf_count(const uint16_t* s, int count, const unsigned (&h)[N], int (&acc)[N]) {
    unsigned w[N];
#pragma unroll
    for (int k = 0; k + 1 < N; ++k) w[k] = s[k];
    for (int j = 0; j < count; ++j) {
        w[N - 1] = s[j + N - 1];
        bool same = true;
#pragma unroll
        for (int k = 0; k < N; ++k) {
            same = same && w[k] == h[k];
            acc[k] += same ? 1 : 0;
        }
#pragma unroll
        for (int k = 0; k + 1 < N; ++k) w[k] = w[k + 1];
    }
}

// matched[k] of the orders k + 1 <= N between the streams sa (na characters, the lanes' own) and sb, summed over the
// wavefront; the orders above N stay 0
template <int N>
__device__ __forceinline__ void chrf_matched(const uint16_t* sa, int na, const uint16_t* sb, int nb, int lane,
                                             int matched[NM_CHRF_MAX_ORDER]) {
    int mine[N];
#pragma unroll
    for (int k = 0; k < N; ++k) mine[k] = 0;
    for (int i = lane; i < na; i += 64) {
        unsigned h[N];
        int before[N], other[N];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            h[k] = sa[i + k];
            before[k] = other[k] = 0;
        }
        chrf_count<N>(sa, i, h, before);
        chrf_count<N>(sb, nb, h, other);
#pragma unroll
        for (int k = 0; k < N; ++k) mine[k] += before[k] < other[k] ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < NM_CHRF_MAX_ORDER; ++k) matched[k] = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) matched[k] = chrf_wave_sum(mine[k]);
}

// Both columns expanded into lds (the reference first) and matched: their lengths and matched[], on every lane.
template <int N>
__device__ __forceinline__ void chrf_pair(uint16_t* lds, const int32_t* rcol, long rstride, int T_ref,
                                          const int32_t* hcol, long hstride, int T_hyp, int end_id,
                                          const ChrfTable& tab, int lane, int& lr, int& lh,
                                          int matched[NM_CHRF_MAX_ORDER]) {
    uint16_t* sr = lds;
    uint16_t* sh = lds + T_ref * (tab.max_word + 1) + CHRF_PAD;
    lr = chrf_expand(sr, rcol, rstride, T_ref, end_id, tab, CHRF_FILL_REF, lane);
    lh = chrf_expand(sh, hcol, hstride, T_hyp, end_id, tab, CHRF_FILL_HYP, lane);
    __syncthreads();                                     // the streams are staged (one wavefront per workgroup)
    const bool hyp_shorter = lh <= lr;
    chrf_matched<N>(hyp_shorter ? sh : sr, hyp_shorter ? lh : lr, hyp_shorter ? sr : sh, hyp_shorter ? lr : lh, lane,
                    matched);
}

// The score from the integers, as SentenceChrF.__call__ states it: in double, the sums in the order m = 1..n, no
// fused multiply-add; the caller's conversion to float is the one rounding.
__device__ __forceinline__ double chrf_score(int n, double beta2, const int matched[NM_CHRF_MAX_ORDER], int lh,
                                             int lr) {
#pragma clang fp contract(off)
    if (lh == 0 || lr == 0) return (lh == 0 && lr == 0) ? 1.0 : 0.0;
    double precision = 0.0, recall = 0.0;
    for (int k = 0; k < n; ++k) {
        const int total_h = max(0, lh - k), total_r = max(0, lr - k);
        precision += total_h > 0 ? (double)matched[k] / (double)total_h : 1.0;
        recall += total_r > 0 ? (double)matched[k] / (double)total_r : 1.0;
    }
    precision /= (double)n;
    recall /= (double)n;
    if (precision == 0.0 && recall == 0.0) return 0.0;
    return (1.0 + beta2) * (precision * recall) / (beta2 * precision + recall);
}

template <int N>
__global__ __launch_bounds__(64) void chrf_reward_kernel(const int32_t* __restrict__ ref, long ref_stride, int T_ref,
                                                         const int32_t* __restrict__ hyp, long hyp_stride, int T_hyp,
                                                         int end_id, ChrfTable tab, double beta2,
                                                         float* __restrict__ reward, int32_t* __restrict__ counts) {
    extern __shared__ uint16_t chrf_lds[];
    const int lane = threadIdx.x;
    const long b = blockIdx.x;                           // one sentence per wavefront
    int lr, lh, matched[NM_CHRF_MAX_ORDER];
    chrf_pair<N>(chrf_lds, ref + b, ref_stride, T_ref, hyp + b, hyp_stride, T_hyp, end_id, tab, lane, lr, lh, matched);
    if (lane == 0) reward[b] = (float)chrf_score(N, beta2, matched, lh, lr);
    if (counts != nullptr && lane < NM_CHRF_MAX_ORDER) {
        int m = 0;
#pragma unroll
        for (int k = 0; k < NM_CHRF_MAX_ORDER; ++k) m = k == lane ? matched[k] : m;
        int32_t* out = counts + b * 3 * NM_CHRF_MAX_ORDER;
        out[lane] = m;
        out[NM_CHRF_MAX_ORDER + lane] = lane < N ? max(0, lh - lane) : 0;
        out[2 * NM_CHRF_MAX_ORDER + lane] = lane < N ? max(0, lr - lane) : 0;
    }
}

// Wavefront u of the grid owns the u-th unordered pair i < j, counted through the sentences: hypothesis sample i against
// reference sample j.  The first B n threads of the grid also write the diagonal, which needs no matching.
template <int N>
__global__ __launch_bounds__(64) void chrf_pairwise_kernel(const int32_t* __restrict__ tok, long t_stride, int T, long B,
                                                           int n, int end_id, ChrfTable tab, double beta2,
                                                           float* __restrict__ U) {
    extern __shared__ uint16_t chrf_lds[];
    const int lane = threadIdx.x;
    const long own = (long)blockIdx.x * 64 + lane;
    if (own < B * n) {
        const long b = own / n, i = own % n;
        U[(b * n + i) * n + i] = 1.0f;
    }
    const long pairs = (long)n * (n - 1) / 2, u = blockIdx.x;
    if (u >= B * pairs) return;                          // the whole wavefront: blockIdx.x is uniform
    const long b = u / pairs;
    int i = 0, j = (int)(u % pairs);                     // pair j of the rows (0,1) .. (0,n-1), (1,2) .. (1,n-1), ...
    while (j >= n - 1 - i) {
        j -= n - 1 - i;
        ++i;
    }
    j += i + 1;
    const int32_t* col = tok + b * n;
    int lr, lh, matched[NM_CHRF_MAX_ORDER];
    chrf_pair<N>(chrf_lds, col + j, t_stride, T, col + i, t_stride, T, end_id, tab, lane, lr, lh, matched);
    float* u_b = U + b * n * n;
    if (lane == 0) u_b[i * n + j] = (float)chrf_score(N, beta2, matched, lh, lr);      // hypothesis i, reference j
    if (lane == 1) u_b[j * n + i] = (float)chrf_score(N, beta2, matched, lr, lh);      // hypothesis j, reference i
}

// LAUNCH(N) for the order n in 1..6
#define CHRF_DISPATCH(n, LAUNCH) \
    do {                         \
        switch (n) {             \
        case 1: LAUNCH(1); break; \
        case 2: LAUNCH(2); break; \
        case 3: LAUNCH(3); break; \
        case 4: LAUNCH(4); break; \
        case 5: LAUNCH(5); break; \
        default: LAUNCH(6); break; \
        }                        \
    } while (0)

// the checks the two entry points share; `what` names the entry point, `tokens` is the sum of the two columns' lengths
int chrf_check(const char* what, int n, double beta, int64_t tokens, int64_t V, int64_t max_word_chars) {
    NM_REQUIRE(n >= 1 && n <= NM_CHRF_MAX_ORDER, "%s: order n %d outside 1..%d", what, n, NM_CHRF_MAX_ORDER);
    NM_REQUIRE(beta > 0.0, "%s: beta %g is not above 0", what, beta);
    NM_REQUIRE(V >= 1 && V < (1ll << 31) && max_word_chars >= 1,
               "%s: bad table sizes V %lld, max_word_chars %lld", what, (long long)V, (long long)max_word_chars);
    NM_REQUIRE(max_word_chars < CHRF_MAX_CHARS && tokens * (max_word_chars + 1) <= CHRF_MAX_CHARS,
               "%s: %lld tokens of up to %lld characters and a space are more than the %d characters the LDS staging "
               "holds", what, (long long)tokens, (long long)max_word_chars, CHRF_MAX_CHARS);
    return NM_OK;
}

size_t chrf_lds_bytes(int64_t tokens, int64_t max_word_chars) {
    return (size_t)(tokens * (max_word_chars + 1) + 2 * CHRF_PAD) * sizeof(uint16_t);
}

}  // namespace

extern "C" {

int64_t nm_chrf_max_chars(void) { return CHRF_MAX_CHARS; }

int nm_chrf_reward(void* stream, const int32_t* ref, int64_t ref_stride, int64_t T_ref, const int32_t* hyp,
                   int64_t hyp_stride, int64_t T_hyp, int64_t B, int32_t end_id, const int32_t* rows,
                   const uint16_t* chars, int64_t V, int64_t max_word_chars, int n, double beta, float* reward,
                   int32_t* counts) {
    NM_REQUIRE(B >= 0 && T_ref >= 1 && T_hyp >= 1, "nm_chrf_reward: bad sizes B %lld, T_ref %lld, T_hyp %lld",
               (long long)B, (long long)T_ref, (long long)T_hyp);
    NM_REQUIRE(T_ref <= CHRF_MAX_CHARS && T_hyp <= CHRF_MAX_CHARS,
               "nm_chrf_reward: T_ref %lld or T_hyp %lld above the %d characters the LDS staging holds",
               (long long)T_ref, (long long)T_hyp, CHRF_MAX_CHARS);
    if (int rc = chrf_check("nm_chrf_reward", n, beta, T_ref + T_hyp, V, max_word_chars)) return rc;
    NM_REQUIRE(ref_stride >= B && hyp_stride >= B, "nm_chrf_reward: row stride %lld or %lld below B = %lld",
               (long long)ref_stride, (long long)hyp_stride, (long long)B);
    NM_REQUIRE(ref_stride < (1ll << 31) / T_ref && hyp_stride < (1ll << 31) / T_hyp,
               "nm_chrf_reward: a token array spans more than 2^31 - 1 elements");
    NM_REQUIRE(B < CHRF_MAX_WAVEFRONTS, "nm_chrf_reward: %lld sentences are more than %d wavefronts in one launch",
               (long long)B, CHRF_MAX_WAVEFRONTS);
    if (B == 0) return NM_OK;
    NM_REQUIRE(ref != nullptr && hyp != nullptr && rows != nullptr && chars != nullptr && reward != nullptr,
               "nm_chrf_reward: null pointer");
    NM_REQUIRE((reinterpret_cast<uintptr_t>(rows) & 15u) == 0, "nm_chrf_reward: rows is not 16-byte aligned");
    const ChrfTable tab = {reinterpret_cast<const int4*>(rows), chars, (int)V, (int)max_word_chars};
#define CHRF_LAUNCH_REWARD(N)                                                                                          \
    hipLaunchKernelGGL((chrf_reward_kernel<N>), dim3((unsigned)B), dim3(64),                                           \
                       chrf_lds_bytes(T_ref + T_hyp, max_word_chars), nm_stream(stream), ref, (long)ref_stride,        \
                       (int)T_ref, hyp, (long)hyp_stride, (int)T_hyp, (int)end_id, tab, beta * beta, reward, counts)
    CHRF_DISPATCH(n, CHRF_LAUNCH_REWARD);
#undef CHRF_LAUNCH_REWARD
    NM_LAUNCH_CHECK("nm_chrf_reward");
}

int nm_chrf_pairwise(void* stream, const int32_t* tok, int64_t t_stride, int64_t T, int64_t B, int64_t n_samples,
                     int32_t end_id, const int32_t* rows, const uint16_t* chars, int64_t V, int64_t max_word_chars,
                     int n, double beta, float* U) {
    NM_REQUIRE(n_samples >= 1 && n_samples <= CHRF_MAX_SAMPLES, "nm_chrf_pairwise: n_samples %lld outside 1..%d",
               (long long)n_samples, CHRF_MAX_SAMPLES);
    NM_REQUIRE(B >= 0 && T >= 1, "nm_chrf_pairwise: bad sizes B %lld, T %lld", (long long)B, (long long)T);
    NM_REQUIRE(T <= CHRF_MAX_CHARS, "nm_chrf_pairwise: T %lld above the %d characters the LDS staging holds",
               (long long)T, CHRF_MAX_CHARS);
    if (int rc = chrf_check("nm_chrf_pairwise", n, beta, 2 * T, V, max_word_chars)) return rc;
    NM_REQUIRE(B < (1ll << 31) / (n_samples * n_samples), "nm_chrf_pairwise: B %lld * n_samples %lld squared beyond "
               "2^31 - 1", (long long)B, (long long)n_samples);
    NM_REQUIRE(t_stride >= B * n_samples, "nm_chrf_pairwise: row stride %lld below B * n_samples = %lld",
               (long long)t_stride, (long long)(B * n_samples));
    NM_REQUIRE(t_stride < (1ll << 31) / T, "nm_chrf_pairwise: the token array spans more than 2^31 - 1 elements");
    const int64_t units = B * (n_samples * (n_samples - 1) / 2), for_diagonal = nm_cdiv(B * n_samples, 64);
    NM_REQUIRE(units < CHRF_MAX_WAVEFRONTS, "nm_chrf_pairwise: %lld pairs are more than %d wavefronts in one launch",
               (long long)units, CHRF_MAX_WAVEFRONTS);
    if (B == 0) return NM_OK;
    NM_REQUIRE(tok != nullptr && rows != nullptr && chars != nullptr && U != nullptr, "nm_chrf_pairwise: null pointer");
    NM_REQUIRE((reinterpret_cast<uintptr_t>(rows) & 15u) == 0, "nm_chrf_pairwise: rows is not 16-byte aligned");
    const ChrfTable tab = {reinterpret_cast<const int4*>(rows), chars, (int)V, (int)max_word_chars};
#define CHRF_LAUNCH_PAIRWISE(N)                                                                                        \
    hipLaunchKernelGGL((chrf_pairwise_kernel<N>), dim3((unsigned)(units > for_diagonal ? units : for_diagonal)),       \
                       dim3(64), chrf_lds_bytes(2 * T, max_word_chars), nm_stream(stream), tok, (long)t_stride, (int)T, \
                       (long)B, (int)n_samples, (int)end_id, tab, beta * beta, U)
    CHRF_DISPATCH(n, CHRF_LAUNCH_PAIRWISE);
#undef CHRF_LAUNCH_PAIRWISE
    NM_LAUNCH_CHECK("nm_chrf_pairwise");
}

}  // extern "C"
