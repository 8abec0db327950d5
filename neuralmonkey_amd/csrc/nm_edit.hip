// Edit-distance scores of sentences (include/nmhip_edit.h): the Levenshtein distance d of a reference and
// a hypothesis column, each cut at its first end token, finished as the edit accuracy 1 - d / max(lr, lh) or as the
// negative word error rate -d / max(lr, 1) -- the reward of minimum-WER self-critical training (nm_edit_reward) and the
// utility of minimum Bayes risk decoding for speech and character-level models (nm_edit_pairwise).
//
// The table D[i][j] (i reference tokens against j hypothesis tokens) depends on its left, upper and upper-left
// neighbours: neither a row nor a column can be split over lanes as it stands.  A pair is therefore swept along its
// anti-diagonals by a SEGMENT of W lanes of one wavefront, W in {16, 32, 64}; a wavefront carries 64 / W pairs.
//
//   columns    lane l of a segment owns the C consecutive hypothesis columns l C + 1 .. l C + C (C in {1, 2, 4, 8, 16},
//              a template parameter): their tokens h[C] and the previous row's values prev[C] stay in registers.  The
//              host takes the smallest W C >= T_hyp: C = 1 up to 64 columns, then W = 64 and the next power of two.
//   reference  staged ONCE in LDS (T_ref words per segment, the lanes also find its end on the way).
//   sweep      skewed: at step s lane l computes reference row s - l + 1 of its strip.  Its left boundary D[i][l C]
//              is the last value lane l - 1 computed one step earlier and arrives by ONE lane shift per step (DPP
//              wave_shr:1, no LDS); the upper-left boundary D[i - 1][l C] is the value the shift brought one step
//              before, kept in a register.  A segment's first lane ignores what the shift brings across the segment
//              boundary and supplies D[i][0] = i itself.  The table never touches LDS and there is no barrier in the
//              loop; the one LDS access of a step is the reference token of the NEXT step, whose address depends on
//              nothing the step computes.  Within a strip the chain through the left neighbour is add + min per cell:
//              min(up + 1, diag + (r != h)) does not depend on it.
//   bounds     a pair runs lr + ceil(lh / C) - 1 steps, not T; a packed wavefront runs the largest count of its
//              segments, a lane outside rows 1 .. lr of its pair holds still.  Columns behind lh compute values nothing
//              reads (D[i][j] depends on columns <= j only).
//   result     after the loop the lane that owns column lh holds D[lr][lh]; lr == 0 or lh == 0 is the other length.
// Integers throughout, double in the one-line finish, no atomics: two runs are bit-equal.
#include "nm_common.h"
#include "../../include/nmhip_edit.h"

namespace {

constexpr int EDIT_MAX_COLUMNS = 16;                     // the largest C
constexpr int EDIT_MAX_TOKENS = 64 * EDIT_MAX_COLUMNS;   // nm_edit_max_tokens()
constexpr int EDIT_MAX_SAMPLES = 64;                     // as nm_mbr_select: one lane per sample there
constexpr int EDIT_MAX_WAVEFRONTS = 1 << 25;             // of one launch: 2^31 threads, which every runtime takes

// 64 / W of EDIT_DISPATCH below
inline int64_t edit_pairs_per_wavefront(int64_t columns) { return columns <= 16 ? 4 : columns <= 32 ? 2 : 1; }

// lane l takes `v` of lane l - 1 of the wavefront (DPP wave_shr:1); lane 0 takes 0
__device__ __forceinline__ int edit_from_lower_lane(int v) {
    return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xf, 0xf, false);
}

// The score of a pair from its integers, in double, rounded once by the caller's conversion to float.
__device__ __forceinline__ double edit_score(int kind, int d, int lr, int lh) {
    if (kind == 0) {
        const int longer = lr > lh ? lr : lh;
        return longer == 0 ? 1.0 : 1.0 - (double)d / (double)longer;
    }
    return (double)(-d) / (double)(lr > 1 ? lr : 1);
}

// The distance of one pair, swept by the segment of W lanes that `lane` belongs to; every lane of the segment returns
// it, with the two lengths in lr and lh.  Called by ALL 64 lanes of the wavefront (the lane shift and the barrier need
// them); a segment without a pair passes valid = false and returns 0 with lr = lh = 0.
//   sref   the segment's T_ref words of LDS;  rcol / hcol  element t of the column at [t * stride]
template <int C, int W>
__device__ __forceinline__ int edit_distance(int32_t* sref, const int32_t* rcol, long rstride, int T_ref,
                                             const int32_t* hcol, long hstride, int T_hyp, bool valid, int end_id,
                                             int lane, int& lr, int& lh) {
    const int sl = lane & (W - 1);                       // the lane within its segment
    int er = valid ? T_ref : 0, eh = valid ? T_hyp : 0;  // the first end token this lane has seen
    if (valid) {
        for (int t = sl; t < T_ref; t += W) {
            const int32_t v = rcol[(long)t * rstride];
            sref[t] = v;
            if (v == end_id && t < er) er = t;
        }
    }
    int32_t h[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int t = sl * C + c;
        int32_t v = 0;
        if (valid && t < T_hyp) {
            v = hcol[(long)t * hstride];
            if (v == end_id && t < eh) eh = t;
        }
        h[c] = v;
    }
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) {          // off < W: the partner is a lane of the same segment
        const int other_r = __shfl_xor(er, off, 64), other_h = __shfl_xor(eh, off, 64);
        er = other_r < er ? other_r : er;
        eh = other_h < eh ? other_h : eh;
    }
    lr = er;
    lh = eh;
    __syncthreads();                                     // the reference is staged (one wavefront per workgroup)

    const int own = (lr > 0 && lh > 0) ? lr + (lh + C - 1) / C - 1 : 0;
    int steps = 0;                                       // of the wavefront: the largest of its segments, uniform
#pragma unroll
    for (int seg = 0; seg < 64 / W; ++seg) {
        const int theirs = __builtin_amdgcn_readlane(own, seg * W);
        steps = theirs > steps ? theirs : steps;
    }

    int prev[C];                                         // D[row - 1][sl C + 1 + c]; row 0 is the column index
#pragma unroll
    for (int c = 0; c < C; ++c) prev[c] = sl * C + c + 1;
    int diag = sl * C;                                   // D[row - 1][sl C]
    int row = 1 - sl;                                    // the reference row (from 1) this lane computes at step 0
    const int last = T_ref - 1;
    int32_t r = sref[row - 1 < 0 ? 0 : row - 1 > last ? last : row - 1];
    for (int s = 0; s < steps; ++s, ++row) {
        const int shifted = edit_from_lower_lane(prev[C - 1]);           // D[row][sl C], computed one step ago
        const int32_t r_next = sref[row < 0 ? 0 : row > last ? last : row];
        if (row >= 1 && row <= lr) {
            int left = sl == 0 ? row : shifted;
            int dg = diag;
            diag = left;                                                 // the next row's upper-left boundary
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int up = prev[c];
                const int open = min(up + 1, dg + (r != h[c] ? 1 : 0));  // does not wait for the left neighbour
                left = min(open, left + 1);
                dg = up;
                prev[c] = left;
            }
        }
        r = r_next;
    }

    int d = prev[0];                                     // D[lr][lh] on the lane that owns column lh
    const int owner = lh > 0 ? (lh - 1) / C : 0, cc = lh > 0 ? (lh - 1) % C : 0;
#pragma unroll
    for (int c = 1; c < C; ++c) d = c == cc ? prev[c] : d;
    d = __shfl(d, (lane & ~(W - 1)) + owner, 64);
    return (lr == 0 || lh == 0) ? lr + lh : d;
}

template <int C, int W>
__global__ __launch_bounds__(64) void edit_reward_kernel(int kind, const int32_t* __restrict__ ref, long ref_stride,
                                                         int T_ref, const int32_t* __restrict__ hyp, long hyp_stride,
                                                         int T_hyp, long B, int end_id, float* __restrict__ reward,
                                                         int32_t* __restrict__ dist) {
    extern __shared__ int32_t edit_lds[];
    const int lane = threadIdx.x, seg = lane / W;
    const long b = (long)blockIdx.x * (64 / W) + seg;    // one sentence per segment
    const bool valid = b < B;
    int lr, lh;
    const int d = edit_distance<C, W>(edit_lds + seg * T_ref, ref + (valid ? b : 0), ref_stride, T_ref,
                                      hyp + (valid ? b : 0), hyp_stride, T_hyp, valid, end_id, lane, lr, lh);
    if (valid && (lane & (W - 1)) == 0) {
        reward[b] = (float)edit_score(kind, d, lr, lh);
        if (dist != nullptr) dist[b] = d;
    }
}

// Segment u of the grid owns the u-th unordered pair i < j, counted through the sentences: hypothesis sample i against
// reference sample j.  The first B n threads of the grid also write the diagonal, which needs no distance.
template <int C, int W>
__global__ __launch_bounds__(64) void edit_pairwise_kernel(int kind, const int32_t* __restrict__ tok, long t_stride,
                                                           int T, long B, int n, int end_id, float* __restrict__ U) {
    extern __shared__ int32_t edit_lds[];
    const int lane = threadIdx.x, seg = lane / W;
    const long own = (long)blockIdx.x * 64 + lane;
    if (own < B * n) {
        const long b = own / n, i = own % n;
        U[(b * n + i) * n + i] = kind == 0 ? 1.0f : 0.0f;
    }
    const long pairs = (long)n * (n - 1) / 2, u = (long)blockIdx.x * (64 / W) + seg;
    const bool valid = u < B * pairs;
    long b = 0;
    int i = 0, j = 0;
    if (valid) {
        b = u / pairs;
        j = (int)(u % pairs);                            // pair j of the rows (0,1) .. (0,n-1), (1,2) .. (1,n-1), ...
        while (j >= n - 1 - i) {
            j -= n - 1 - i;
            ++i;
        }
        j += i + 1;
    }
    const int32_t* col = tok + b * n;
    int lr, lh;
    const int d = edit_distance<C, W>(edit_lds + seg * T, col + j, t_stride, T, col + i, t_stride, T, valid, end_id,
                                      lane, lr, lh);
    const int sl = lane & (W - 1);
    if (valid && sl < 2) {                               // two lanes finish the two directions
        float* u_b = U + b * n * n;
        if (sl == 0) u_b[i * n + j] = (float)edit_score(kind, d, lr, lh);      // hypothesis i, reference j
        else u_b[j * n + i] = (float)edit_score(kind, d, lh, lr);              // hypothesis j, reference i
    }
}

// LAUNCH(C, W) for the smallest W * C >= columns
#define EDIT_DISPATCH(columns, LAUNCH)          \
    do {                                        \
        if ((columns) <= 16) LAUNCH(1, 16);     \
        else if ((columns) <= 32) LAUNCH(1, 32);  \
        else if ((columns) <= 64) LAUNCH(1, 64);  \
        else if ((columns) <= 128) LAUNCH(2, 64); \
        else if ((columns) <= 256) LAUNCH(4, 64); \
        else if ((columns) <= 512) LAUNCH(8, 64); \
        else LAUNCH(16, 64);                    \
    } while (0)

}  // namespace

extern "C" {

int64_t nm_edit_max_tokens(void) { return EDIT_MAX_TOKENS; }

int nm_edit_reward(void* stream, int kind, const int32_t* ref, int64_t ref_stride, int64_t T_ref, const int32_t* hyp,
                   int64_t hyp_stride, int64_t T_hyp, int64_t B, int32_t end_id, float* reward, int32_t* dist) {
    NM_REQUIRE(kind == 0 || kind == 1, "nm_edit_reward: kind %d (0 edit accuracy, 1 negative WER)", kind);
    NM_REQUIRE(B >= 0 && T_ref >= 1 && T_hyp >= 1, "nm_edit_reward: bad sizes B %lld, T_ref %lld, T_hyp %lld",
               (long long)B, (long long)T_ref, (long long)T_hyp);
    NM_REQUIRE(T_ref <= EDIT_MAX_TOKENS && T_hyp <= EDIT_MAX_TOKENS,
               "nm_edit_reward: T_ref %lld or T_hyp %lld above the %d tokens a wavefront's registers hold",
               (long long)T_ref, (long long)T_hyp, EDIT_MAX_TOKENS);
    NM_REQUIRE(ref_stride >= B && hyp_stride >= B, "nm_edit_reward: row stride %lld or %lld below B = %lld",
               (long long)ref_stride, (long long)hyp_stride, (long long)B);
    NM_REQUIRE(ref_stride < (1ll << 31) / T_ref && hyp_stride < (1ll << 31) / T_hyp,
               "nm_edit_reward: a token array spans more than 2^31 - 1 elements");
    NM_REQUIRE(B / edit_pairs_per_wavefront(T_hyp) < EDIT_MAX_WAVEFRONTS,
               "nm_edit_reward: %lld sentences are more than %d wavefronts in one launch", (long long)B,
               EDIT_MAX_WAVEFRONTS);
    if (B == 0) return NM_OK;
    NM_REQUIRE(ref != nullptr && hyp != nullptr && reward != nullptr, "nm_edit_reward: null pointer");
#define EDIT_LAUNCH_REWARD(C, W)                                                                                      \
    do {                                                                                                              \
        hipLaunchKernelGGL((edit_reward_kernel<C, W>), dim3((unsigned)nm_cdiv(B, 64 / W)), dim3(64),                  \
                           (size_t)(64 / W) * T_ref * sizeof(int32_t), nm_stream(stream), kind, ref,                  \
                           (long)ref_stride, (int)T_ref, hyp, (long)hyp_stride, (int)T_hyp, (long)B, (int)end_id,     \
                           reward, dist);                                                                             \
    } while (0)
    EDIT_DISPATCH(T_hyp, EDIT_LAUNCH_REWARD);
#undef EDIT_LAUNCH_REWARD
    NM_LAUNCH_CHECK("nm_edit_reward");
}

int nm_edit_pairwise(void* stream, int kind, const int32_t* tok, int64_t t_stride, int64_t T, int64_t B, int64_t n,
                     int32_t end_id, float* U) {
    NM_REQUIRE(kind == 0 || kind == 1, "nm_edit_pairwise: kind %d (0 edit accuracy, 1 negative WER)", kind);
    NM_REQUIRE(n >= 1 && n <= EDIT_MAX_SAMPLES, "nm_edit_pairwise: n %lld samples outside 1..%d", (long long)n,
               EDIT_MAX_SAMPLES);
    NM_REQUIRE(B >= 0 && T >= 1, "nm_edit_pairwise: bad sizes B %lld, T %lld", (long long)B, (long long)T);
    NM_REQUIRE(T <= EDIT_MAX_TOKENS, "nm_edit_pairwise: T %lld above the %d tokens a wavefront's registers hold",
               (long long)T, EDIT_MAX_TOKENS);
    NM_REQUIRE(B < (1ll << 31) / (n * n), "nm_edit_pairwise: B %lld * n %lld * n beyond 2^31 - 1", (long long)B,
               (long long)n);
    NM_REQUIRE(t_stride >= B * n, "nm_edit_pairwise: row stride %lld below B * n = %lld", (long long)t_stride,
               (long long)(B * n));
    NM_REQUIRE(t_stride < (1ll << 31) / T, "nm_edit_pairwise: the token array spans more than 2^31 - 1 elements");
    const int64_t units = B * (n * (n - 1) / 2), diagonal = B * n;
    NM_REQUIRE(units / edit_pairs_per_wavefront(T) < EDIT_MAX_WAVEFRONTS,
               "nm_edit_pairwise: %lld pairs are more than %d wavefronts in one launch", (long long)units,
               EDIT_MAX_WAVEFRONTS);
    if (B == 0) return NM_OK;
    NM_REQUIRE(tok != nullptr && U != nullptr, "nm_edit_pairwise: null pointer");
#define EDIT_LAUNCH_PAIRWISE(C, W)                                                                                    \
    do {                                                                                                              \
        const int for_pairs = nm_cdiv(units, 64 / W), for_diagonal = nm_cdiv(diagonal, 64);                           \
        hipLaunchKernelGGL((edit_pairwise_kernel<C, W>), dim3((unsigned)(for_pairs > for_diagonal ? for_pairs         \
                                                                                                 : for_diagonal)),    \
                           dim3(64), (size_t)(64 / W) * T * sizeof(int32_t), nm_stream(stream), kind, tok,            \
                           (long)t_stride, (int)T, (long)B, (int)n, (int)end_id, U);                                  \
    } while (0)
    EDIT_DISPATCH(T, EDIT_LAUNCH_PAIRWISE);
#undef EDIT_LAUNCH_PAIRWISE
    NM_LAUNCH_CHECK("nm_edit_pairwise");
}

}  // extern "C"
