// CTC prefix beam search (include/nmhip_ctc_beam.h): tf.nn.ctc_beam_search_decoder with top_paths = 1 on the
// logits rows x[t, b, 0..K) of nm_ctc.hip (explicit t and b strides, class K-1 the blank), log-space fp32, beams of 1 to 64.
//
//   cbs_rows_kernel   one wave per (t, b) row, the row read ONCE: the online log-sum-exp of ctc_row_stats_kernel and, in
//                     the same pass, the M = min(beam + 1, K - 1) non-blank classes of largest logit.  The select is a
//                     threshold filter: a class whose (logit, lower class first) key beats the threshold is appended to
//                     a 256-entry LDS list by ballot + popcount; when the list could overflow it is sorted (bitonic, 64-bit
//                     keys), cut to M and its M-th key becomes the threshold.  Keys are unique, so the result does not
//                     depend on the order of the appends.  Out: lse, lp[blank], M (class, lp) pairs in descending order.
//   cbs_scan_kernel   one wave per sentence walks its frames; beam slot i lives in lane i (pb, pl, tot, the prefix's
//                     identity and its parent's, tree node, last label in registers, mirrored in LDS for the other
//                     lanes).  Per frame a lane finds its parent's slot by identity, forms its survivor, and owns the extensions of its prefix as a CURSOR into the
//                     row's short list, which is already in descending order for it: only the class equal to its last
//                     label (lowered: it continues from pb alone) is held apart, and the classes whose extension is in
//                     the beam are struck out of a 65-bit mask by their lanes (integer atomicOr in LDS).  Selection is a
//                     64-way merge: every round each lane offers the best of its survivor, its held-apart class and its
//                     cursor, a wave maximum over (tot', survivor, slot) keys takes one, the winner writes beam slot r
//                     and, for an extension, a (parent, label) node of the sentence's tree.  No candidate matrix exists:
//                     LDS holds the beam (1.5 KiB), the short list and the masks.  The tail walks the best node's
//                     parents twice (count, then write in place from the end), dropping repeats when asked.
// Nothing is summed across lanes in an order that could change, and nothing returns to the host between frames.
#include "nm_common.h"
#include "../../include/nmhip_ctc_beam.h"

namespace {

constexpr int CBS_MAX_BEAM = 64;
constexpr int CBS_LIST = 256;              // entries of the row pass's candidate list
constexpr int64_t CBS_MAX_GRID = 1 << 20;  // workgroups of the row pass; each walks the rows r, r + grid, ...

struct CbsWs {
    float* lse;                            // [B*T], row b*T + t
    float* lpb;                            // [B*T] lp[blank]
    int32_t* top_cls;                      // [B*T, M]
    float* top_lp;                         // [B*T, M]
    int2* arena;                           // [B, 1 + T*beam] (parent node, label); node 0 is the empty prefix
};

inline int64_t cbs_align(int64_t bytes) { return (bytes + 255) / 256 * 256; }
inline int64_t cbs_short(int64_t K, int64_t beam) { return beam + 1 < K - 1 ? beam + 1 : K - 1; }

int64_t cbs_layout(int64_t B, int64_t T, int64_t K, int64_t beam, void* base, CbsWs* ws) {
    const int64_t M = cbs_short(K, beam);
    char* p = static_cast<char*>(base);
    int64_t off = 0;
    auto take = [&](int64_t bytes) { char* q = p ? p + off : nullptr; off += cbs_align(bytes); return q; };
    char* lse = take(B * T * 4);
    char* lpb = take(B * T * 4);
    char* cls = take(B * T * M * 4);
    char* lp = take(B * T * M * 4);
    char* arena = take(B * (1 + T * beam) * 8);
    if (ws) {
        ws->lse = reinterpret_cast<float*>(lse);
        ws->lpb = reinterpret_cast<float*>(lpb);
        ws->top_cls = reinterpret_cast<int32_t*>(cls);
        ws->top_lp = reinterpret_cast<float*>(lp);
        ws->arena = reinterpret_cast<int2*>(arena);
    }
    return off;
}

__device__ __forceinline__ int cbs_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// a float as an unsigned integer of the same order (and back)
__device__ __forceinline__ unsigned cbs_key(float s) {
    const unsigned u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float cbs_unkey(unsigned k) {
    return (k & 0x80000000u) ? __uint_as_float(k & 0x7fffffffu) : __uint_as_float(~k);
}

__device__ __forceinline__ unsigned long long cbs_wave_max(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

// log(exp(a) + exp(b)), -inf when both are (the exp / log of nm_ctc.hip)
__device__ __forceinline__ float cbs_lae(float a, float b) {
    const float m = fmaxf(a, b);
    if (m == -INFINITY) return -INFINITY;
    return m + __logf(__expf(a - m) + __expf(b - m));
}

// The identity of a prefix is a 64-bit hash of its labels, h(p + k) = mix(h(p) + (k + 1) * odd): a prefix that left the
// beam and is extended into again is the same prefix (TensorFlow keeps one trie entry per prefix for that), which tree
// node numbers would not show.  mix is a bijection (the splitmix64 finaliser), so the children of one prefix never
// share a value; two unrelated prefixes of one beam do with probability 2^-64 per pair.
constexpr unsigned long long CBS_ROOT = 0x9e3779b97f4a7c15ull;
__device__ __forceinline__ unsigned long long cbs_child(unsigned long long h, int k) {
    unsigned long long z = h + (unsigned long long)(k + 1) * 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// a tree node other lanes of this wave wrote earlier in the kernel: read past the vector cache
__device__ __forceinline__ int2 cbs_node(const int2* arena, int id) {
    const int* p = reinterpret_cast<const int*>(arena + id);
    return make_int2(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                     __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// buf[0..n) into descending order, n a power of two; the workgroup is ONE wave, so the barriers cost nothing
__device__ __forceinline__ void cbs_sort_desc(unsigned long long* buf, int n, int lane) {
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = lane; p < (n >> 1); p += 64) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
                const unsigned long long a = buf[i], c = buf[l];
                if ((a < c) == ((i & k) == 0)) { buf[i] = c; buf[l] = a; }
            }
            __syncthreads();
        }
}

// ---- row pass -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void cbs_rows_kernel(const float* __restrict__ x, int64_t st, int64_t sb, int T, int K,
                                                      int64_t rows, const int32_t* __restrict__ frame_len, int M,
                                                      float* __restrict__ lse_out, float* __restrict__ lpb_out,
                                                      int32_t* __restrict__ top_cls, float* __restrict__ top_lp) {
    __shared__ unsigned long long buf[CBS_LIST];
    const int lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {         // row b*T + t
    const int b = (int)(r / T), t = (int)(r % T);
    if (t >= cbs_clamp(frame_len[b], 0, T)) continue;                // frames past the length are never read
    const float* row = x + (int64_t)t * st + (int64_t)b * sb;
    __syncthreads();                                                 // the row before is done with the list
#pragma unroll
    for (int q = 0; q < CBS_LIST / 64; ++q) buf[q * 64 + lane] = 0ull;
    unsigned long long thr = 0ull;                                   // the M-th best key so far (0: fewer than M seen)
    int count = 0;                                                   // wave-uniform
    float m = -INFINITY, s = 0.0f;
    for (int base = 0; base < K; base += 256) {
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = base + q * 64 + lane;
            v[q] = k < K ? row[k] : -INFINITY;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = base + q * 64 + lane;
            if (base + q * 64 >= K) break;
            if (k < K) {
                if (v[q] > m) {
                    s = s * __expf(m - v[q]) + 1.0f;
                    m = v[q];
                } else if (v[q] > -INFINITY) {
                    s += __expf(v[q] - m);
                }
            }
            // (logit, lower class first) as one integer; never 0 for a class, and no two classes share a key
            const unsigned long long comp =
                k < K - 1 ? ((unsigned long long)cbs_key(v[q]) << 32) | (unsigned)(0x7fffffff - k) : 0ull;
            const bool pass = comp > thr;
            const unsigned long long mask = __ballot(pass);
            if (pass) buf[count + __popcll(mask & below)] = comp;
            count += __popcll(mask);
            if (count > CBS_LIST - 64) {                             // the next 64 classes might not fit: cut to M
                __syncthreads();
                cbs_sort_desc(buf, CBS_LIST, lane);
                if (count > M) {
                    thr = buf[M - 1];
                    __syncthreads();
                    for (int i = M + lane; i < count; i += 64) buf[i] = 0ull;
                    count = M;
                }
                __syncthreads();
            }
        }
    }
    __syncthreads();
    cbs_sort_desc(buf, count <= 64 ? 64 : (count <= 128 ? 128 : CBS_LIST), lane);
    const float mm = nm_wave_max(m);
    const float tot = nm_wave_sum(m == -INFINITY ? 0.0f : s * __expf(m - mm));
    const float lse = mm + __logf(tot);
    if (lane == 0) {
        lse_out[r] = lse;
        lpb_out[r] = row[K - 1] - lse;
    }
    for (int j = lane; j < M; j += 64) {
        const unsigned long long comp = buf[j];
        const bool have = comp != 0ull;                              // (K - 1 >= M classes were offered: always)
        top_cls[r * M + j] = have ? 0x7fffffff - (int)(unsigned)(comp & 0xffffffffull) : 0;
        top_lp[r * M + j] = have ? cbs_unkey((unsigned)(comp >> 32)) - lse : -INFINITY;
    }
    }
}

// ---- frame scan and backtrack ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void cbs_scan_kernel(const float* __restrict__ x, int64_t st, int64_t sb, int T,
                                                      const int32_t* __restrict__ frame_len, int beam, int M, int merge,
                                                      int end_token, const float* __restrict__ lse,
                                                      const float* __restrict__ lpb, const int32_t* __restrict__ top_cls,
                                                      const float* __restrict__ top_lp, int2* __restrict__ arena_all,
                                                      int32_t* __restrict__ tokens, int32_t* __restrict__ out_len,
                                                      float* __restrict__ score) {
    __shared__ float s_pb[64], s_pl[64], s_tot[64];
    __shared__ unsigned long long s_hid[64], s_hpar[64];           // prefix identities of the slots and of their parents
    __shared__ int s_node[64], s_last[64];
    __shared__ int s_cls[CBS_MAX_BEAM + 1];
    __shared__ float s_lp[CBS_MAX_BEAM + 1];
    __shared__ unsigned long long s_m0[64];                          // struck-out short-list entries 0..63 of slot i
    __shared__ unsigned s_m1[64];                                    // ... and entry 64
    const int b = blockIdx.x, lane = threadIdx.x;
    const int len = cbs_clamp(frame_len[b], 0, T);
    const float* xb = x + (int64_t)b * sb;
    int2* arena = arena_all + (int64_t)b * (1 + (int64_t)T * beam);
    const int64_t r0 = (int64_t)b * T;
    int32_t* out = tokens + (int64_t)b * T;

    // beam slot `lane`: the empty prefix in slot 0
    float pb = lane == 0 ? 0.0f : -INFINITY, pl = -INFINITY, tot = pb;
    unsigned long long hid = CBS_ROOT, hpar = 0ull;
    int node = lane == 0 ? 0 : -1, last = -1;
    int nbeam = 1, nnodes = 1;
    s_pb[lane] = pb; s_pl[lane] = pl; s_tot[lane] = tot;
    s_hid[lane] = hid; s_hpar[lane] = hpar; s_node[lane] = node; s_last[lane] = last;
    if (lane == 0) arena[0] = make_int2(-1, -1);

    // frame 0's short list in flight; a frame's list is fetched while the frame before it is searched
    int ncls0 = 0, ncls1 = 0;
    float nlp0 = -INFINITY, nlp1 = -INFINITY, nlpb = 0.0f, nlse = 0.0f, xg = 0.0f;
    if (len > 0) {
        if (lane < M) { ncls0 = top_cls[r0 * M + lane]; nlp0 = top_lp[r0 * M + lane]; }
        if (M > 64) { ncls1 = top_cls[r0 * M + 64]; nlp1 = top_lp[r0 * M + 64]; }
        nlpb = lpb[r0];
        nlse = lse[r0];
    }
    for (int t = 0; t < len; ++t) {
        __syncthreads();                                             // the frame before is done with the list and the beam
        if (lane < M) { s_cls[lane] = ncls0; s_lp[lane] = nlp0; }
        if (M > 64 && lane == 0) { s_cls[64] = ncls1; s_lp[64] = nlp1; }
        s_m0[lane] = M < 64 ? ~0ull << M : 0ull;
        s_m1[lane] = M > 64 ? 0u : 1u;
        const float lpb_t = nlpb, lse_t = nlse;
        const float x_last = xg;                                     // x[t, b, last], asked for when the beam was formed
        __syncthreads();
        if (t + 1 < len) {
            const int64_t rn = r0 + t + 1;
            if (lane < M) { ncls0 = top_cls[rn * M + lane]; nlp0 = top_lp[rn * M + lane]; }
            if (M > 64) { ncls1 = top_cls[rn * M + 64]; nlp1 = top_lp[rn * M + 64]; }
            nlpb = lpb[rn];
            nlse = lse[rn];
        }
        const bool active = lane < nbeam;

        // the parent prefix's slot, and where this prefix's last label stands in the short list
        int pslot = -1, jm = -1;
        for (int j = 0; j < nbeam; ++j)
            if (active && last >= 0 && s_hid[j] == hpar) pslot = j;
        for (int j = 0; j < M; ++j)
            if (active && s_cls[j] == last) jm = j;
        float prev = -INFINITY;
        if (pslot >= 0) prev = s_last[pslot] == last ? s_pb[pslot] : s_tot[pslot];
        if (pslot >= 0 && jm >= 0) {                                 // parent + last is this prefix: no extension of it
            if (jm < 64) atomicOr(&s_m0[pslot], 1ull << jm);
            else atomicOr(&s_m1[pslot], 1u);
        }
        __syncthreads();
        unsigned long long m0 = s_m0[lane];
        unsigned m1 = s_m1[lane];

        // survivor
        const float spb = tot + lpb_t;
        const float spl = last >= 0 ? (x_last - lse_t) + cbs_lae(pl, prev) : -INFINITY;
        float sv = active ? cbs_lae(spb, spl) : -INFINITY;
        // the extension by the last label continues from pb alone: held apart from the cursor
        float spec_v = -INFINITY;
        if (jm >= 0) {
            const bool struck = jm < 64 ? (m0 >> jm) & 1ull : m1 & 1u;
            if (!struck) spec_v = s_lp[jm] + pb;
            if (jm < 64) m0 |= 1ull << jm; else m1 |= 1u;
        }
        // cursor: the first entry at or after `from` that is not struck out
        int head = -1;
        float head_v = -INFINITY;
        auto advance = [&](int from) {
            const unsigned long long open = from < 64 ? ~m0 & (~0ull << from) : 0ull;
            head = open ? __ffsll((long long)open) - 1 : ((from <= 64 && !(m1 & 1u)) ? 64 : -1);
            head_v = (active && head >= 0) ? s_lp[head] + tot : -INFINITY;
        };
        advance(0);
        const unsigned long long hid_old = hid, hpar_old = hpar;
        const int node_old = node, last_old = last;
        __syncthreads();                                             // every lane has read the old beam

        int r = 0;
        for (; r < beam; ++r) {
            // this lane's offer: 0 survivor, 1 cursor, 2 held-apart class (ties: survivor, then the lower class)
            int kind = 0;
            float v = sv;
            if (head_v > v) { kind = 1; v = head_v; }
            if (spec_v > v || (kind == 1 && spec_v == v && jm < head)) { kind = 2; v = spec_v; }
            const unsigned long long offer =
                v > -INFINITY ? ((unsigned long long)cbs_key(v) << 32) | (unsigned)((kind == 0 ? 64 : 0) | (63 - lane))
                              : 0ull;
            const unsigned long long best = cbs_wave_max(offer);
            if (best == 0ull) break;                                 // fewer candidates than beam slots
            const bool ext = !(best & 64ull);
            if (offer == best) {                                     // one lane: the slot bits differ
                if (kind == 0) {
                    s_pb[r] = spb; s_pl[r] = spl; s_tot[r] = sv;
                    s_hid[r] = hid_old; s_hpar[r] = hpar_old; s_node[r] = node_old; s_last[r] = last_old;
                    sv = -INFINITY;
                } else {
                    const int j = kind == 1 ? head : jm;
                    const int c = s_cls[j];
                    s_pb[r] = -INFINITY; s_pl[r] = v; s_tot[r] = v;
                    s_hid[r] = cbs_child(hid_old, c); s_hpar[r] = hid_old; s_node[r] = nnodes; s_last[r] = c;
                    arena[nnodes] = make_int2(node_old, c);
                    if (kind == 1) advance(head + 1); else spec_v = -INFINITY;
                }
            }
            nnodes += ext ? 1 : 0;
        }
        nbeam = r;
        __syncthreads();
        const bool now = lane < nbeam;
        pb = now ? s_pb[lane] : -INFINITY;
        pl = now ? s_pl[lane] : -INFINITY;
        tot = now ? s_tot[lane] : -INFINITY;
        hid = s_hid[lane];
        hpar = s_hpar[lane];
        node = now ? s_node[lane] : -1;
        last = now ? s_last[lane] : -1;
        xg = (t + 1 < len && last >= 0) ? xb[(int64_t)(t + 1) * st + last] : 0.0f;
        if (nbeam == 0) break;                                       // (only when a frame holds no finite value)
    }

    // the best prefix is in slot 0: the rounds took the candidates in descending order
    __threadfence();
    __syncthreads();
    int count = 0;
    if (lane == 0 && len > 0 && nbeam > 0) {
        for (int pass = 0; pass < 2; ++pass) {
            int pos = count, id = node, kept = 0;
            int2 cur = id > 0 ? cbs_node(arena, id) : make_int2(-1, -1);
            while (id > 0) {
                const int2 up = cur.x > 0 ? cbs_node(arena, cur.x) : make_int2(-1, -1);
                if (!(merge && cur.x > 0 && up.y == cur.y)) {
                    ++kept;
                    if (pass == 1) out[--pos] = cur.y;
                }
                id = cur.x;
                cur = up;
            }
            count = kept;
        }
    }
    count = __shfl(count, 0, 64);
    for (int i = count + lane; i < T; i += 64) out[i] = end_token;
    if (lane == 0) {
        out_len[b] = count;
        score[b] = (len > 0 && nbeam > 0) ? tot : 0.0f;
    }
}

int cbs_check_shape(const char* fn, int64_t T, int64_t B, int64_t K, int64_t beam) {
    NM_REQUIRE(T >= 0 && B >= 0, "%s: negative size (T %lld, B %lld)", fn, (long long)T, (long long)B);
    NM_REQUIRE(K >= 2, "%s: at least one class beside the blank (K >= 2), got K = %lld", fn, (long long)K);
    NM_REQUIRE(beam >= 1 && beam <= CBS_MAX_BEAM, "%s: beam_size must be between 1 and %d, got %lld", fn, CBS_MAX_BEAM,
               (long long)beam);
    NM_REQUIRE(T * B < (1ll << 31) - 4 && K < (1ll << 31) - 256 && T * beam < (1ll << 31) - 4 &&
                   T * B * (beam + 1) < (1ll << 40),
               "%s: sizes beyond 32-bit row and node counts", fn);
    return NM_OK;
}

}  // namespace

extern "C" {

int64_t nm_ctc_beam_workspace_bytes(int64_t B, int64_t T, int64_t K, int64_t beam_size) {
    if (cbs_check_shape("nm_ctc_beam_workspace_bytes", T, B, K, beam_size)) return -1;
    return cbs_layout(B, T, K, beam_size, nullptr, nullptr);
}

int nm_ctc_beam_search(void* stream, const float* logits, int64_t stride_t, int64_t stride_b, int64_t T, int64_t B,
                       int64_t K, const int32_t* frame_len, int64_t beam_size, int merge_repeated, int32_t end_token,
                       int32_t* tokens, int32_t* out_len, float* score, void* workspace, int64_t workspace_bytes) {
    if (int rc = cbs_check_shape("nm_ctc_beam_search", T, B, K, beam_size)) return rc;
    if (B == 0) return NM_OK;
    NM_REQUIRE(frame_len != nullptr && out_len != nullptr && score != nullptr && workspace != nullptr,
               "nm_ctc_beam_search: null pointer (frame_len, out_len, score or workspace)");
    NM_REQUIRE(T == 0 || (logits != nullptr && tokens != nullptr), "nm_ctc_beam_search: null pointer (logits or tokens)");
    NM_REQUIRE(stride_t >= 0 && stride_b >= 0, "nm_ctc_beam_search: negative stride");
    CbsWs ws;
    const int64_t need = cbs_layout(B, T, K, beam_size, workspace, &ws);
    if (workspace_bytes < need)
        NM_FAIL(NM_ERR_WORKSPACE, "nm_ctc_beam_search: workspace too small (%lld < %lld bytes)",
                (long long)workspace_bytes, (long long)need);
    hipStream_t s = nm_stream(stream);
    const int M = (int)cbs_short(K, beam_size);
    if (T > 0)
        hipLaunchKernelGGL(cbs_rows_kernel, dim3((unsigned)(T * B < CBS_MAX_GRID ? T * B : CBS_MAX_GRID)), dim3(64), 0, s,
                           logits, stride_t, stride_b, (int)T, (int)K, T * B, frame_len, M, ws.lse, ws.lpb, ws.top_cls, ws.top_lp);
    hipLaunchKernelGGL(cbs_scan_kernel, dim3((unsigned)B), dim3(64), 0, s, logits, stride_t, stride_b, (int)T, frame_len,
                       (int)beam_size, M, merge_repeated ? 1 : 0, (int)end_token, ws.lse, ws.lpb, ws.top_cls, ws.top_lp,
                       ws.arena, tokens, out_len, score);
    NM_LAUNCH_CHECK("nm_ctc_beam_search");
}

}  // extern "C"
