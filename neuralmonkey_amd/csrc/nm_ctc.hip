// Connectionist temporal classification (include/nmhip_ctc.h): loss, gradient of the logits and greedy decoding of
// decoders/ctc_decoder.py (tf.nn.ctc_loss / tf.nn.ctc_greedy_decoder), log-space fp32.
//
// The logits are rows x[t, b, 0..K) addressed with explicit t and b strides (the encoder's states are batch-major, no
// transposed copy is made); class K-1 is the blank.  With l' the labels of a sentence with blanks interleaved
// (S = 2L+1 states) and lp the log-softmax emissions:
//   ctc_row_stats_kernel     one wave per (t, b) row: log-sum-exp and / or argmax (ties: lowest class)
//   ctc_alpha_beta_kernel    two workgroups per sentence run the alpha and the beta recursion side by side (beta does
//                            not depend on alpha): states across lanes, two LDS rows ping-ponged, ONE barrier per frame,
//                            the lp[t+1, l'[u]] gather of the next frame in flight across it
//   ctc_grad_kernel          one workgroup per (t, b) row: scale * (softmax - occupancy); the states' posteriors are
//                            normalised by their sum over the frame, and the states of one class are summed in a fixed
//                            order (the thread of a label's first occurrence walks the later ones; one wave sums the
//                            blanks), so two runs are bit-equal -- no floating-point atomics
//   ctc_greedy_kernel        one wave per sentence compacts the frames' argmax classes (ballot + popcount)
// Workspace rows: lse / argmax [B*T] (row b*T + t), alpha / beta [B, T, 2 Lmax + 1].
#include "nm_common.h"

namespace {

constexpr int CTC_MAX_LABELS = 3000;       // 2 (2 Lmax + 3) floats + Lmax ints of LDS stay under 64 KiB

struct CtcWs {
    float* lse;
    float* alpha;
    float* beta;
    float* logz;
    int32_t* valid;
    int32_t* first;
    int32_t* next;
    int32_t* argmax;
};

inline int64_t ctc_align(int64_t bytes) { return (bytes + 255) / 256 * 256; }

int64_t ctc_layout(int64_t B, int64_t T, int64_t Lmax, void* base, CtcWs* ws) {
    const int64_t S = 2 * Lmax + 1;
    char* p = static_cast<char*>(base);
    int64_t off = 0;
    auto take = [&](int64_t bytes) { char* q = p ? p + off : nullptr; off += ctc_align(bytes); return q; };
    char* lse = take(B * T * 4);
    char* alpha = take(B * T * S * 4);
    char* beta = take(B * T * S * 4);
    char* logz = take(B * 4);
    char* valid = take(B * 4);
    char* first = take(B * Lmax * 4);
    char* next = take(B * Lmax * 4);
    char* argmax = take(B * T * 4);
    if (ws) {
        ws->lse = reinterpret_cast<float*>(lse);
        ws->alpha = reinterpret_cast<float*>(alpha);
        ws->beta = reinterpret_cast<float*>(beta);
        ws->logz = reinterpret_cast<float*>(logz);
        ws->valid = reinterpret_cast<int32_t*>(valid);
        ws->first = reinterpret_cast<int32_t*>(first);
        ws->next = reinterpret_cast<int32_t*>(next);
        ws->argmax = reinterpret_cast<int32_t*>(argmax);
    }
    return off;
}

__device__ __forceinline__ int ctc_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// log(exp(a) + exp(b) + exp(c)); -inf when all three are (v_exp / v_log are quarter rate: this is the inner cost)
__device__ __forceinline__ float ctc_lse3(float a, float b, float c) {
    const float m = fmaxf(a, fmaxf(b, c));
    if (m == -INFINITY) return -INFINITY;
    return m + __logf(__expf(a - m) + __expf(b - m) + __expf(c - m));
}

// ---- row statistics ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ctc_row_stats_kernel(const float* __restrict__ x, int64_t st, int64_t sb, int T,
                                                            int B, int K, const int32_t* __restrict__ frame_len,
                                                            float* __restrict__ lse, int32_t* __restrict__ argmax) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= (int64_t)T * B) return;
    const int b = (int)(r / T), t = (int)(r % T);
    if (t >= ctc_clamp(frame_len[b], 0, T)) return;                  // wave-uniform: frames past the length are never read
    const float* row = x + (int64_t)t * st + (int64_t)b * sb;
    float m = -INFINITY, s = 0.0f, bv = -INFINITY;
    int best = K;
#pragma unroll 4
    for (int k = lane; k < K; k += 64) {
        const float v = row[k];
        if (v > bv || best == K) { bv = v; best = k; }
        if (v > m) {
            s = s * __expf(m - v) + 1.0f;
            m = v;
        } else if (v > -INFINITY) {
            s += __expf(v - m);
        }
    }
    if (lse != nullptr) {
        const float mm = nm_wave_max(m);
        const float tot = nm_wave_sum(m == -INFINITY ? 0.0f : s * __expf(m - mm));
        if (lane == 0) lse[r] = mm + __logf(tot);
    }
    if (argmax != nullptr) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(best, off, 64);
            if (oi < K && (best == K || ov > bv || (ov == bv && oi < best))) { bv = ov; best = oi; }
        }
        if (lane == 0) argmax[r] = best;
    }
}

// ---- the two recursions -------------------------------------------------------------------------------------------
// blockIdx.y == 0: alpha_t(u) = lp(t, u) + log sum of the allowed predecessors' alpha_{t-1}; stores alpha, the
// sentence's log Z / loss / validity and the same-class links of its labels.  blockIdx.y == 1: the tail sums
// bs_t(u) = log sum of the allowed successors' (lp(t+1, .) + bs_{t+1}(.)), stored WITHOUT the state's own emission,
// so the posterior of (t, u) is exp(alpha + bs - log Z) with no gather in the gradient pass.
__global__ __launch_bounds__(1024) void ctc_alpha_beta_kernel(
    const float* __restrict__ x, int64_t st, int64_t sb, int T, int K, const int32_t* __restrict__ labels, int Lmax,
    const int32_t* __restrict__ label_len, const int32_t* __restrict__ frame_len, int merge,
    const float* __restrict__ lse, float* __restrict__ alpha, float* __restrict__ beta, float* __restrict__ logz,
    int32_t* __restrict__ valid, int32_t* __restrict__ first, int32_t* __restrict__ next, float* __restrict__ loss) {
    extern __shared__ float ctc_smem[];
    __shared__ int s_rep, s_bad;
    const int b = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x, nt = blockDim.x;
    const int Smax = 2 * Lmax + 1;
    float* buf0 = ctc_smem;
    float* buf1 = ctc_smem + (Smax + 2);
    int* lab = reinterpret_cast<int*>(ctc_smem + 2 * (Smax + 2));
    const int L = ctc_clamp(label_len[b], 0, Lmax);
    const int len = ctc_clamp(frame_len[b], 0, T);
    const int S = 2 * L + 1, blank = K - 1;
    if (tid == 0) { s_rep = 0; s_bad = 0; }
    for (int i = tid; i < L; i += nt) lab[i] = labels[(int64_t)b * Lmax + i];
    __syncthreads();
    int rep = 0, bad = 0;
    for (int i = tid; i < L; i += nt) {
        const int c = lab[i];
        if (c < 0 || c >= blank) bad = 1;
        if (i > 0 && c == lab[i - 1]) rep++;
    }
    if (rep) atomicAdd(&s_rep, rep);
    if (bad) atomicOr(&s_bad, 1);
    __syncthreads();
    // ignore_longer_outputs_than_inputs: a sentence needs a frame per label and, when repeated outputs merge, a blank
    // between equal neighbours; an empty label sequence is valid (the all-blank path), zero frames are not
    const bool ok = !s_bad && len >= 1 && L + (merge ? s_rep : 0) <= len;
    if (dir == 0) {
        for (int i = tid; i < L; i += nt) {
            const int c = lab[i];
            int f = 1, n = -1;
            for (int j = 0; j < i; ++j)
                if (lab[j] == c) { f = 0; break; }
            for (int j = i + 1; j < L; ++j)
                if (lab[j] == c) { n = j; break; }
            first[(int64_t)b * Lmax + i] = f;
            next[(int64_t)b * Lmax + i] = n;
        }
        if (tid == 0 && !ok) {
            valid[b] = 0;
            logz[b] = 0.0f;
            loss[b] = s_bad ? NAN : 0.0f;                          // a label outside [0, K-1) is the caller's error
        }
    }
    if (!ok) return;

    const float* xb = x + (int64_t)b * sb;
    const float* lse_b = lse + (int64_t)b * T;
    const int u0 = tid;
    const bool has = u0 < S;
    const int cls0 = (has && (u0 & 1)) ? lab[u0 >> 1] : blank;
    const bool self0 = merge || !(u0 & 1);
    float* prev = buf0;
    float* cur = buf1;

    if (dir == 0) {
        float* a_out = alpha + (int64_t)b * T * Smax;
        const bool skip0 = has && (u0 & 1) && u0 >= 3 && !(merge && lab[u0 >> 1] == lab[(u0 >> 1) - 1]);
        if (tid < 2) { buf0[tid] = -INFINITY; buf1[tid] = -INFINITY; }      // states -2, -1
        for (int u = tid; u < S; u += nt) {
            const int cls = (u & 1) ? lab[u >> 1] : blank;
            const float v = u < 2 ? xb[cls] - lse_b[0] : -INFINITY;
            buf0[u + 2] = v;
            a_out[u] = v;
        }
        float e_next = (has && len > 1) ? xb[st + cls0] - lse_b[1] : 0.0f;
        for (int t = 1; t < len; ++t) {
            __syncthreads();
            const float* xt = xb + (int64_t)t * st;
            float* arow = a_out + (int64_t)t * Smax;
            if (has) {
                const float v = e_next + ctc_lse3(self0 ? prev[u0 + 2] : -INFINITY, prev[u0 + 1],
                                                  skip0 ? prev[u0] : -INFINITY);
                cur[u0 + 2] = v;
                arow[u0] = v;
            }
            for (int u = tid + nt; u < S; u += nt) {               // more states than threads
                const int odd = u & 1, cls = odd ? lab[u >> 1] : blank;
                const bool skip = odd && !(merge && lab[u >> 1] == lab[(u >> 1) - 1]);
                const float v = xt[cls] - lse_b[t] + ctc_lse3((merge || !odd) ? prev[u + 2] : -INFINITY, prev[u + 1],
                                                              skip ? prev[u] : -INFINITY);
                cur[u + 2] = v;
                arow[u] = v;
            }
            if (has && t + 1 < len) e_next = xt[st + cls0] - lse_b[t + 1];   // in flight across the next barrier
            float* tmp = prev; prev = cur; cur = tmp;
        }
        __syncthreads();
        if (tid == 0) {
            const float lz = ctc_lse3(prev[S - 1 + 2], S > 1 ? prev[S - 2 + 2] : -INFINITY, -INFINITY);
            const bool fin = lz > -INFINITY && lz < INFINITY;
            valid[b] = fin ? 1 : 0;
            logz[b] = fin ? lz : 0.0f;
            loss[b] = fin ? -lz : 0.0f;
        }
    } else {
        float* b_out = beta + (int64_t)b * T * Smax;
        const bool skip0 = has && (u0 & 1) && u0 + 2 < S && !(merge && lab[(u0 >> 1) + 1] == lab[u0 >> 1]);
        if (tid < 2) { buf0[S + tid] = -INFINITY; buf1[S + tid] = -INFINITY; }   // states S, S+1
        {
            const float* xt = xb + (int64_t)(len - 1) * st;
            float* brow = b_out + (int64_t)(len - 1) * Smax;
            for (int u = tid; u < S; u += nt) {
                const int cls = (u & 1) ? lab[u >> 1] : blank;
                const float bs = u >= S - 2 ? 0.0f : -INFINITY;
                buf0[u] = u >= S - 2 ? xt[cls] - lse_b[len - 1] : -INFINITY;
                brow[u] = bs;
            }
        }
        float e_next = (has && len > 1) ? xb[(int64_t)(len - 2) * st + cls0] - lse_b[len - 2] : 0.0f;
        for (int t = len - 2; t >= 0; --t) {
            __syncthreads();
            const float* xt = xb + (int64_t)t * st;
            float* brow = b_out + (int64_t)t * Smax;
            if (has) {
                const float bs = ctc_lse3(self0 ? prev[u0] : -INFINITY, prev[u0 + 1], skip0 ? prev[u0 + 2] : -INFINITY);
                cur[u0] = e_next + bs;
                brow[u0] = bs;
            }
            for (int u = tid + nt; u < S; u += nt) {
                const int odd = u & 1, cls = odd ? lab[u >> 1] : blank;
                const bool skip = odd && u + 2 < S && !(merge && lab[(u >> 1) + 1] == lab[u >> 1]);
                const float bs = ctc_lse3((merge || !odd) ? prev[u] : -INFINITY, prev[u + 1],
                                          skip ? prev[u + 2] : -INFINITY);
                cur[u] = xt[cls] - lse_b[t] + bs;
                brow[u] = bs;
            }
            if (has && t > 0) e_next = xb[(int64_t)(t - 1) * st + cls0] - lse_b[t - 1];
            float* tmp = prev; prev = cur; cur = tmp;
        }
    }
}

__global__ __launch_bounds__(256) void ctc_loss_sum_kernel(const float* __restrict__ loss, int B,
                                                           float* __restrict__ loss_sum) {
    __shared__ float part[256];
    float acc = 0.0f;
    for (int b = threadIdx.x; b < B; b += 256) acc += loss[b];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss_sum[0] = part[0];
}

// ---- gradient of the logits -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ctc_grad_kernel(
    const float* x, int64_t st, int64_t sb, int T, int K, const int32_t* __restrict__ labels, int Lmax,
    const int32_t* __restrict__ label_len, const int32_t* __restrict__ frame_len, const float* __restrict__ scale,
    float* dl, int64_t dst, int64_t dsb, const float* __restrict__ lse, const float* __restrict__ alpha,
    const float* __restrict__ beta, const float* __restrict__ logz, const int32_t* __restrict__ valid,
    const int32_t* __restrict__ first, const int32_t* __restrict__ next) {
    extern __shared__ float ctc_post[];                            // posterior of every state of this frame
    __shared__ float s_part[4];
    const int64_t r = blockIdx.x;                                  // row b*T + t
    const int b = (int)(r / T), t = (int)(r % T);
    const int tid = threadIdx.x, nt = blockDim.x;
    float* drow = dl + (int64_t)t * dst + (int64_t)b * dsb;
    if (!valid[b] || t >= ctc_clamp(frame_len[b], 0, T)) {          // exact zeros: no alignment, or past the length
        for (int k = tid; k < K; k += nt) drow[k] = 0.0f;
        return;
    }
    const float* xrow = x + (int64_t)t * st + (int64_t)b * sb;
    const int Smax = 2 * Lmax + 1;
    const int L = ctc_clamp(label_len[b], 0, Lmax), S = 2 * L + 1;
    const float sc = scale != nullptr ? scale[0] : 1.0f;
    const float lz = logz[b], l = lse[r];
    const float* arow = alpha + r * Smax;
    const float* brow = beta + r * Smax;
    // posterior of the states, normalised by THIS frame's sum over the states instead of exp(log Z): in exact
    // arithmetic the two agree, in fp32 the rounding error alpha and beta have gathered over the frames (an ulp of
    // |alpha| ~ T log K per step, common to the states of a frame) cancels
    float part = 0.0f;
    for (int u = tid; u < S; u += nt) {
        const float e = __expf(arow[u] + brow[u] - lz);
        ctc_post[u] = e;
        part += e;
    }
    part = nm_wave_sum(part);
    if ((tid & 63) == 0) s_part[tid >> 6] = part;
#pragma unroll 4
    for (int k = tid; k < K; k += nt) drow[k] = sc * __expf(xrow[k] - l);       // (in place: same thread, same element)
    __syncthreads();
    float tot = 0.0f;
    for (int w = 0; w < (nt >> 6); ++w) tot += s_part[w];
    const float sci = tot > 0.0f ? sc / tot : 0.0f;
    const int32_t* lab = labels + (int64_t)b * Lmax;
    const int32_t* fst = first + (int64_t)b * Lmax;
    const int32_t* nxt = next + (int64_t)b * Lmax;
    for (int i = tid; i < L; i += nt) {
        if (!fst[i]) continue;
        float occ = 0.0f;
        for (int j = i; j >= 0; j = nxt[j]) occ += ctc_post[2 * j + 1];
        drow[lab[i]] -= sci * occ;
    }
    if (tid >= nt - 64) {                                          // the last wave: the blanks, even states
        const int lane = tid & 63;
        float occ = 0.0f;
        for (int u = 2 * lane; u < S; u += 128) occ += ctc_post[u];
        occ = nm_wave_sum(occ);
        if (lane == 0) drow[K - 1] -= sci * occ;
    }
}

// ---- greedy decoding ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void ctc_greedy_kernel(const int32_t* __restrict__ argmax, int T, int K,
                                                        const int32_t* __restrict__ frame_len, int merge, int end_token,
                                                        int32_t* __restrict__ tokens, int32_t* __restrict__ out_len) {
    const int b = blockIdx.x, lane = threadIdx.x, blank = K - 1;
    const int len = ctc_clamp(frame_len[b], 0, T);
    const int32_t* am = argmax + (int64_t)b * T;
    int32_t* out = tokens + (int64_t)b * T;
    int count = 0;
    for (int base = 0; base < len; base += 64) {
        const int t = base + lane;
        const int c = t < len ? am[t] : blank;
        const int p = (t > 0 && t < len) ? am[t - 1] : -1;          // the previous FRAME's class, blanks included
        const bool emit = t < len && c != blank && !(merge && c == p);
        const unsigned long long mask = __ballot(emit);
        if (emit) out[count + __popcll(mask & ((1ull << lane) - 1ull))] = c;
        count += __popcll(mask);
    }
    for (int t = count + lane; t < T; t += 64) out[t] = end_token;
    if (lane == 0) out_len[b] = count;
}

__global__ __launch_bounds__(256) void ctc_mask_lengths_kernel(const float* __restrict__ mask, int64_t ld, int B, int T,
                                                               int32_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    float acc = 0.0f;
    for (int t = lane; t < T; t += 64) acc += mask[(int64_t)b * ld + t];
    acc = nm_wave_sum(acc);
    if (lane == 0) out[b] = (int)rintf(acc);
}

int ctc_check_shape(const char* fn, int64_t T, int64_t B, int64_t K, int64_t Lmax) {
    NM_REQUIRE(T >= 0 && B >= 0 && K >= 1 && Lmax >= 0, "%s: negative size (T %lld, B %lld, K %lld, Lmax %lld)", fn,
               (long long)T, (long long)B, (long long)K, (long long)Lmax);
    NM_REQUIRE(Lmax <= CTC_MAX_LABELS, "%s: at most %d labels per sentence, got %lld", fn, CTC_MAX_LABELS,
               (long long)Lmax);
    NM_REQUIRE(T * B < (1ll << 31) - 4 && K < (1ll << 31) - 64 && B <= 0x7fffffffll / (Lmax + 1),
               "%s: sizes beyond 32-bit row counts", fn);
    return NM_OK;
}

}  // namespace

extern "C" {

int64_t nm_ctc_workspace_bytes(int64_t B, int64_t T, int64_t Lmax) {
    if (B < 0 || T < 0 || Lmax < 0) return -1;
    return ctc_layout(B, T, Lmax, nullptr, nullptr);
}

int nm_ctc_mask_lengths(void* stream, const float* mask, int64_t ld, int64_t B, int64_t T, int32_t* lengths) {
    NM_REQUIRE(B >= 0 && T >= 0 && ld >= T, "nm_ctc_mask_lengths: bad shape (B %lld, T %lld, ld %lld)", (long long)B,
               (long long)T, (long long)ld);
    if (B == 0) return NM_OK;
    NM_REQUIRE(mask != nullptr && lengths != nullptr, "nm_ctc_mask_lengths: null pointer");
    NM_REQUIRE(B < (1ll << 31) - 4 && T < (1ll << 31), "nm_ctc_mask_lengths: sizes beyond 32-bit row counts");
    hipLaunchKernelGGL(ctc_mask_lengths_kernel, dim3(nm_cdiv(B, 4)), dim3(256), 0, nm_stream(stream), mask, ld, (int)B,
                       (int)T, lengths);
    NM_LAUNCH_CHECK("nm_ctc_mask_lengths");
}

int nm_ctc_loss_fwd(void* stream, const float* logits, int64_t stride_t, int64_t stride_b, int64_t T, int64_t B,
                    int64_t K, const int32_t* labels, int64_t Lmax, const int32_t* label_len, const int32_t* frame_len,
                    int merge_repeated, float* loss, float* loss_sum, void* workspace, int64_t workspace_bytes) {
    if (int rc = ctc_check_shape("nm_ctc_loss_fwd", T, B, K, Lmax)) return rc;
    NM_REQUIRE(loss_sum != nullptr, "nm_ctc_loss_fwd: null pointer (loss_sum)");
    NM_REQUIRE(B == 0 || (label_len != nullptr && frame_len != nullptr && loss != nullptr && workspace != nullptr),
               "nm_ctc_loss_fwd: null pointer (label_len, frame_len, loss or workspace)");
    NM_REQUIRE(B == 0 || T == 0 || logits != nullptr, "nm_ctc_loss_fwd: null pointer (logits)");
    NM_REQUIRE(B == 0 || Lmax == 0 || labels != nullptr, "nm_ctc_loss_fwd: null pointer (labels)");
    NM_REQUIRE(stride_t >= 0 && stride_b >= 0, "nm_ctc_loss_fwd: negative stride");
    CtcWs ws;
    const int64_t need = ctc_layout(B, T, Lmax, workspace, &ws);
    if (workspace_bytes < need)
        NM_FAIL(NM_ERR_WORKSPACE, "nm_ctc_loss_fwd: workspace too small (%lld < %lld bytes)", (long long)workspace_bytes,
                (long long)need);
    hipStream_t s = nm_stream(stream);
    if (B > 0) {
        if (T > 0)
            hipLaunchKernelGGL(ctc_row_stats_kernel, dim3(nm_cdiv(T * B, 4)), dim3(256), 0, s, logits, stride_t, stride_b,
                               (int)T, (int)B, (int)K, frame_len, ws.lse, (int32_t*)nullptr);
        const int64_t smax = 2 * Lmax + 1;
        int threads = (int)((smax + 63) / 64 * 64);
        threads = threads > 1024 ? 1024 : threads;
        const size_t lds = (size_t)(2 * (smax + 2) + Lmax) * 4;
        hipLaunchKernelGGL(ctc_alpha_beta_kernel, dim3((unsigned)B, 2), dim3(threads), lds, s, logits, stride_t, stride_b,
                           (int)T, (int)K, labels, (int)Lmax, label_len, frame_len, merge_repeated ? 1 : 0, ws.lse,
                           ws.alpha, ws.beta, ws.logz, ws.valid, ws.first, ws.next, loss);
    }
    hipLaunchKernelGGL(ctc_loss_sum_kernel, dim3(1), dim3(256), 0, s, loss, (int)B, loss_sum);
    NM_LAUNCH_CHECK("nm_ctc_loss_fwd");
}

int nm_ctc_loss_bwd(void* stream, const float* logits, int64_t stride_t, int64_t stride_b, int64_t T, int64_t B,
                    int64_t K, const int32_t* labels, int64_t Lmax, const int32_t* label_len, const int32_t* frame_len,
                    const float* scale, float* dlogits, int64_t dstride_t, int64_t dstride_b, const void* workspace,
                    int64_t workspace_bytes) {
    if (int rc = ctc_check_shape("nm_ctc_loss_bwd", T, B, K, Lmax)) return rc;
    if (B == 0 || T == 0) return NM_OK;
    NM_REQUIRE(logits != nullptr && dlogits != nullptr && label_len != nullptr && frame_len != nullptr &&
                   workspace != nullptr,
               "nm_ctc_loss_bwd: null pointer (logits, dlogits, label_len, frame_len or workspace)");
    NM_REQUIRE(Lmax == 0 || labels != nullptr, "nm_ctc_loss_bwd: null pointer (labels)");
    NM_REQUIRE(stride_t >= 0 && stride_b >= 0 && dstride_t >= 0 && dstride_b >= 0, "nm_ctc_loss_bwd: negative stride");
    CtcWs ws;
    const int64_t need = ctc_layout(B, T, Lmax, const_cast<void*>(workspace), &ws);
    if (workspace_bytes < need)
        NM_FAIL(NM_ERR_WORKSPACE, "nm_ctc_loss_bwd: workspace too small (%lld < %lld bytes)", (long long)workspace_bytes,
                (long long)need);
    const int threads = K <= 512 ? 64 : 256;
    hipLaunchKernelGGL(ctc_grad_kernel, dim3((unsigned)(T * B)), dim3(threads), (size_t)(2 * Lmax + 1) * 4,
                       nm_stream(stream), logits, stride_t, stride_b, (int)T, (int)K, labels, (int)Lmax, label_len,
                       frame_len, scale, dlogits, dstride_t, dstride_b, ws.lse, ws.alpha, ws.beta, ws.logz, ws.valid,
                       ws.first, ws.next);
    NM_LAUNCH_CHECK("nm_ctc_loss_bwd");
}

int nm_ctc_greedy(void* stream, const float* logits, int64_t stride_t, int64_t stride_b, int64_t T, int64_t B, int64_t K,
                  const int32_t* frame_len, int merge_repeated, int32_t end_token, int32_t* tokens, int32_t* out_len,
                  void* workspace, int64_t workspace_bytes) {
    if (int rc = ctc_check_shape("nm_ctc_greedy", T, B, K, 0)) return rc;
    if (B == 0) return NM_OK;
    NM_REQUIRE(frame_len != nullptr && out_len != nullptr && workspace != nullptr,
               "nm_ctc_greedy: null pointer (frame_len, out_len or workspace)");
    NM_REQUIRE(T == 0 || (logits != nullptr && tokens != nullptr), "nm_ctc_greedy: null pointer (logits or tokens)");
    NM_REQUIRE(stride_t >= 0 && stride_b >= 0, "nm_ctc_greedy: negative stride");
    CtcWs ws;
    const int64_t need = ctc_layout(B, T, 0, workspace, &ws);
    if (workspace_bytes < need)
        NM_FAIL(NM_ERR_WORKSPACE, "nm_ctc_greedy: workspace too small (%lld < %lld bytes)", (long long)workspace_bytes,
                (long long)need);
    hipStream_t s = nm_stream(stream);
    if (T > 0)
        hipLaunchKernelGGL(ctc_row_stats_kernel, dim3(nm_cdiv(T * B, 4)), dim3(256), 0, s, logits, stride_t, stride_b,
                           (int)T, (int)B, (int)K, frame_len, (float*)nullptr, ws.argmax);
    hipLaunchKernelGGL(ctc_greedy_kernel, dim3((unsigned)B), dim3(64), 0, s, ws.argmax, (int)T, (int)K, frame_len,
                       merge_repeated ? 1 : 0, (int)end_token, tokens, out_len);
    NM_LAUNCH_CHECK("nm_ctc_greedy");
}

}  // extern "C"
