// Truncated sampling step (include/nmhip_sample.h): temperature, top-k and nucleus sampling with the
// log-probability of every draw, one workgroup per row.
//
// The kept set is a prefix of the row in (z descending, column ascending) order, so it is described by a threshold
// key T and a number of ties: an entry is kept when key(z) > T, or key(z) == T and fewer than `ties` equal entries
// stand in lower columns.  T is found without sorting, by a descent over LDS histograms of (count, mass) per bin:
//   level 0   256 bins of the distance to the row maximum, floor((max - z) * 16): weakly monotone in z, so a bin is
//             a contiguous stretch of the order, and real logits spread over many bins (the atomics do not pile up
//             on the two or three exponent values that the leading byte of a float would give);
//   level 1-4 the four bytes of the order-preserving integer key of z, most significant first, over the entries of
//             the bin (and key prefix) chosen so far: exact on fp32 values.
// Top-k walks the levels by count, the nucleus by mass; the level-0 histogram serves both.  Masses are sums of the
// fixed-point terms round(exp(z - max) * 2^31) in 64-bit integers (V < 2^30 terms of at most 2^31): integer addition
// is associative, so LDS atomics give the same sums in every run and the nucleus boundary is reproducible.
// The row is staged in LDS once (z = x * inv_temperature; up to 36864 columns = 144 KiB of the CU's 160 KiB) and
// every pass reads it there; longer rows are re-read from memory by every pass.
#include "nm_common.h"
#include "../../include/nmhip_sample.h"

#define SAMPLE_NT 1024
#define SAMPLE_NW (SAMPLE_NT / 64)
#define SAMPLE_LDS_MAX_V 36864
#define SAMPLE_SCALE 2147483648.0f

typedef unsigned long long smp_u64;

struct SampleArgs {
    const float* x;
    long ldx;
    int V;
    float inv_t;
    int top_k;            // 0: off
    float top_p;
    const uint32_t* salt_base;
    uint32_t salt_step;
    int end_id;
    const int32_t* finished;
    const float* logprob_sum;
    const int32_t* lengths;
    int32_t* out_symbol;
    float* out_logprob;
    int32_t* out_kept;
    int32_t* out_finished;
    float* out_logprob_sum;
    int32_t* out_lengths;
    int32_t* all_finished;
};

struct SampleSel {
    uint32_t bin, excl_cnt, bin_cnt, total_cnt;
    smp_u64 excl_mass, bin_mass, total_mass;
};

// the hash of gumbel_argmax_kernel (csrc/nm_logits.hip), restated by oracle/nm_oracle.py:gumbel_noise
__device__ __forceinline__ uint32_t smp_mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x21f0aaadu;
    x ^= x >> 15;
    x *= 0x735a2d97u;
    x ^= x >> 15;
    return x;
}

// larger z <=> larger key, equal fp32 values <=> equal keys (-0 counts as +0); NaN sorts behind everything
__device__ __forceinline__ uint32_t smp_key(float z) {
    if (z != z) return 0u;
    if (z == 0.0f) z = 0.0f;
    const uint32_t b = __float_as_uint(z);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ int smp_bin0(float z, float mx) {
    const float t = (mx - z) * 16.0f;
    return (t < 255.0f) ? (int)t : 255;               // NaN (NaN entries, infinite maxima) -> the last bin
}

__device__ __forceinline__ uint32_t smp_term(float z, float mx) {
    float e = (z == mx) ? 1.0f : expf(z - mx);        // (an infinite maximum: inf - inf is not a number)
    e = (e >= 0.0f) ? e : 0.0f;
    return __float2uint_rn(e * SAMPLE_SCALE);
}

// Bins in ascending index = descending z.  Finds the bin b with excl(b) < need <= incl(b), by count or by mass, and the
// totals; every thread of the workgroup calls it, the result is in *sel after the closing barrier.
__device__ __forceinline__ void smp_select(const uint32_t* hc, const smp_u64* hm, bool by_mass, uint32_t need_cnt,
                                           smp_u64 need_mass, uint32_t* wc, smp_u64* wm, SampleSel* sel) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    uint32_t c = 0, ic = 0;
    smp_u64 m = 0, im = 0;
    if (tid < 256) {                                  // waves 0..3, all lanes
        c = ic = hc[tid];
        m = im = hm[tid];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t oc = __shfl_up(ic, off);
            const smp_u64 om = __shfl_up(im, off);
            if (lane >= off) { ic += oc; im += om; }
        }
        if (lane == 63) { wc[w] = ic; wm[w] = im; }
    }
    __syncthreads();
    if (tid < 256) {
        for (int j = 0; j < w; ++j) { ic += wc[j]; im += wm[j]; }
        const uint32_t ec = ic - c;
        const smp_u64 em = im - m;
        const bool hit = by_mass ? (em < need_mass && need_mass <= im) : (ec < need_cnt && need_cnt <= ic);
        if (hit) { sel->bin = tid; sel->excl_cnt = ec; sel->bin_cnt = c; sel->excl_mass = em; sel->bin_mass = m; }
        if (tid == 255) { sel->total_cnt = ic; sel->total_mass = im; }
    }
    __syncthreads();
}

template <bool STAGED>
__device__ __forceinline__ float smp_z(const float* zrow, const float* row, float inv_t, int c) {
    return STAGED ? zrow[c] : __fmul_rn(row[c], inv_t);
}

// The descent: on return the threshold key T, how many entries equal it (n_eq) with their common term, and the count
// and mass of the entries strictly in front of them; need_cnt / need_mass are what is still wanted from the ties.
template <bool STAGED>
__device__ __forceinline__ void smp_descend(const float* zrow, const float* row, float inv_t, int V, float mx,
                                            const uint32_t* h0c, const smp_u64* h0m, uint32_t* h1c, smp_u64* h1m,
                                            uint32_t* wc, smp_u64* wm, SampleSel* sel, bool by_mass,
                                            uint32_t& need_cnt, smp_u64& need_mass, uint32_t& T, uint32_t& n_eq,
                                            smp_u64& term_t, uint32_t& cnt_above, smp_u64& mass_above) {
    const int tid = threadIdx.x;
    smp_select(h0c, h0m, by_mass, need_cnt, need_mass, wc, wm, sel);
    const int b0 = (int)sel->bin;
    cnt_above = sel->excl_cnt;
    mass_above = sel->excl_mass;
    need_cnt -= sel->excl_cnt;
    need_mass -= sel->excl_mass;
    uint32_t prefix = 0;
    for (int lvl = 1; lvl <= 4; ++lvl) {
        if (tid < 256) { h1c[tid] = 0; h1m[tid] = 0; }
        __syncthreads();
        const int sh = 32 - 8 * lvl;
        for (int c = tid; c < V; c += SAMPLE_NT) {
            const float z = smp_z<STAGED>(zrow, row, inv_t, c);
            if (smp_bin0(z, mx) != b0) continue;
            const uint32_t key = smp_key(z);
            if (lvl > 1 && (key >> (sh + 8)) != prefix) continue;
            const int d = 255 - (int)((key >> sh) & 255u);
            atomicAdd(&h1c[d], 1u);
            atomicAdd(&h1m[d], (smp_u64)smp_term(z, mx));
        }
        __syncthreads();
        smp_select(h1c, h1m, by_mass, need_cnt, need_mass, wc, wm, sel);
        prefix = (prefix << 8) | (255u - sel->bin);
        cnt_above += sel->excl_cnt;
        mass_above += sel->excl_mass;
        need_cnt -= sel->excl_cnt;
        need_mass -= sel->excl_mass;
        n_eq = sel->bin_cnt;
        term_t = n_eq ? sel->bin_mass / n_eq : 0;      // equal keys have equal terms
    }
    T = prefix;
}

template <bool STAGED>
__global__ __launch_bounds__(SAMPLE_NT) void sample_step_kernel(SampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) float zrow[];          // [V] when STAGED
    __shared__ uint32_t h0c[256], h1c[256];
    __shared__ smp_u64 h0m[256], h1m[256];
    __shared__ uint32_t wc[SAMPLE_NW];
    __shared__ smp_u64 wm[SAMPLE_NW];
    __shared__ float redf[SAMPLE_NW];
    __shared__ int redi[SAMPLE_NW];
    __shared__ SampleSel sel;
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int V = a.V;
    const float inv_t = a.inv_t;
    const int fin = a.finished[r];
    const float lps = a.logprob_sum[r];
    const int len = a.lengths[r];
    if (fin) {                                        // <pad>, nothing added, the state copied through
        if (tid == 0) {
            a.out_symbol[r] = 0;
            a.out_logprob[r] = 0.0f;
            a.out_kept[r] = 0;
            a.out_finished[r] = 1;
            a.out_logprob_sum[r] = lps;
            a.out_lengths[r] = len;
        }
        return;
    }
    const float* row = a.x + (long)r * a.ldx;

    // ---- pass 0: z = x * inv_temperature into LDS, the row maximum (NaN entries are ignored by fmaxf)
    float mx = -INFINITY;
    if (STAGED) {
        int head = (int)((4u - (uint32_t)((reinterpret_cast<uintptr_t>(row) >> 2) & 3u)) & 3u);
        head = head < V ? head : V;
        if (tid < head) {
            const float z = __fmul_rn(row[tid], inv_t);
            zrow[tid] = z;
            mx = fmaxf(mx, z);
        }
        const int nv4 = (V - head) >> 2;
        const float4* r4 = reinterpret_cast<const float4*>(row + head);
        for (int q = tid; q < nv4; q += SAMPLE_NT) {
            const float4 v = r4[q];
            const float z0 = __fmul_rn(v.x, inv_t), z1 = __fmul_rn(v.y, inv_t);
            const float z2 = __fmul_rn(v.z, inv_t), z3 = __fmul_rn(v.w, inv_t);
            float* dst = zrow + head + 4 * q;
            dst[0] = z0; dst[1] = z1; dst[2] = z2; dst[3] = z3;
            mx = fmaxf(fmaxf(mx, fmaxf(z0, z1)), fmaxf(z2, z3));
        }
        const int tail0 = head + 4 * nv4;
        if (tid < V - tail0) {
            const float z = __fmul_rn(row[tail0 + tid], inv_t);
            zrow[tail0 + tid] = z;
            mx = fmaxf(mx, z);
        }
    } else {
        for (int c = tid; c < V; c += SAMPLE_NT) mx = fmaxf(mx, __fmul_rn(row[c], inv_t));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    if (lane == 0) redf[w] = mx;
    __syncthreads();
    for (int j = 0; j < SAMPLE_NW; ++j) mx = fmaxf(mx, redf[j]);
    __syncthreads();                                  // redf is used again by the argmax below

    // ---- the kept set: threshold key, ties kept, size, mass
    const bool k_on = a.top_k >= 1 && a.top_k < V;
    const bool p_on = a.top_p < 1.0f;
    const bool all = !(k_on || p_on);
    uint32_t T = 0, ties = 0, n_eq = 0;
    int kept = V;
    smp_u64 mass_s = 0;
    if (!all) {
        if (tid < 256) { h0c[tid] = 0; h0m[tid] = 0; }
        __syncthreads();
        for (int c = tid; c < V; c += SAMPLE_NT) {
            const float z = smp_z<STAGED>(zrow, row, inv_t, c);
            const int b = smp_bin0(z, mx);
            atomicAdd(&h0c[b], 1u);
            atomicAdd(&h0m[b], (smp_u64)smp_term(z, mx));
        }
        __syncthreads();
        uint32_t cnt_above = 0, need_cnt = 0;
        smp_u64 mass_above = 0, term_t = 0, need_mass = 0, M;
        if (k_on) {
            need_cnt = (uint32_t)a.top_k;
            smp_descend<STAGED>(zrow, row, inv_t, V, mx, h0c, h0m, h1c, h1m, wc, wm, &sel, false, need_cnt, need_mass,
                                T, n_eq, term_t, cnt_above, mass_above);
            ties = need_cnt;                          // what the entries in front of the ties left of top_k
            M = mass_above + (smp_u64)ties * term_t;
            kept = a.top_k;
            mass_s = M;
        } else {
            smp_select(h0c, h0m, false, 1u, 0, wc, wm, &sel);
            M = sel.total_mass;
            __syncthreads();                          // everyone has read sel before the descent writes it again
        }
        if (p_on) {
            if (M == 0) {                             // no entry has a mass (a row of NaN): the first entry alone
                T = 0; ties = 1; n_eq = 2; kept = 1; mass_s = 0;
            } else {
                const double want = ceil((double)a.top_p * (double)M);
                smp_u64 target = (smp_u64)want;
                target = target < 1 ? 1 : (target > M ? M : target);
                need_mass = target;
                need_cnt = 0;
                smp_descend<STAGED>(zrow, row, inv_t, V, mx, h0c, h0m, h1c, h1m, wc, wm, &sel, true, need_cnt,
                                    need_mass, T, n_eq, term_t, cnt_above, mass_above);
                smp_u64 j = term_t ? (need_mass + term_t - 1) / term_t : 1;
                j = j < 1 ? 1 : (j > n_eq ? n_eq : j);
                ties = (uint32_t)j;
                int kp = (int)(cnt_above + ties);
                kept = (k_on && kp > a.top_k) ? a.top_k : kp;
                mass_s = mass_above + j * term_t;
            }
        }
    }

    // ---- the draw over the kept set: gumbel_argmax_kernel's expression and tie rule
    const uint32_t salt = *a.salt_base + a.salt_step;
    const uint32_t hkey = smp_mix32(salt + (uint32_t)r * 0x85EBCA6Bu);
    float best = -INFINITY;
    int bi = 0;                                       // a row of NaN / -inf logits still yields a valid symbol
    smp_u64 msum = 0;
    if (all || ties >= n_eq) {                        // every tie is kept: membership is key >= T
        for (int c = tid; c < V; c += SAMPLE_NT) {
            const float z = smp_z<STAGED>(zrow, row, inv_t, c);
            if (all) msum += smp_term(z, mx);
            else if (smp_key(z) < T) continue;
            const uint32_t bits = smp_mix32((uint32_t)c * 0x9E3779B1u + hkey);
            const float u = ((float)(bits >> 9) + 0.5f) * (1.0f / 8388608.0f);
            const float v = z - logf(-logf(u));
            if (v > best) { best = v; bi = c; }
        }
    } else {                                          // the first `ties` of the equal entries, in column order
        uint32_t seen = 0;
        for (int c0 = 0; c0 < V; c0 += SAMPLE_NT) {
            const int c = c0 + tid;
            const bool in = c < V;
            const float z = in ? smp_z<STAGED>(zrow, row, inv_t, c) : 0.0f;
            const uint32_t key = smp_key(z);
            const bool eq = in && key == T;
            const smp_u64 bal = __ballot(eq);
            if (lane == 0) wc[w] = (uint32_t)__popcll(bal);
            __syncthreads();
            uint32_t before = seen, tot = 0;
            for (int j = 0; j < SAMPLE_NW; ++j) {
                const uint32_t n = wc[j];
                before += j < w ? n : 0u;
                tot += n;
            }
            before += (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
            seen += tot;
            __syncthreads();
            if (in && (key > T || (eq && before < ties))) {
                const uint32_t bits = smp_mix32((uint32_t)c * 0x9E3779B1u + hkey);
                const float u = ((float)(bits >> 9) + 0.5f) * (1.0f / 8388608.0f);
                const float v = z - logf(-logf(u));
                if (v > best) { best = v; bi = c; }
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(best, off);
        const int oi = __shfl_xor(bi, off);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
        msum += __shfl_xor(msum, off);
    }
    if (lane == 0) { redf[w] = best; redi[w] = bi; wm[w] = msum; }
    __syncthreads();
    if (tid == 0) {
        msum = 0;
        for (int j = 0; j < SAMPLE_NW; ++j) {
            if (j > 0 && (redf[j] > best || (redf[j] == best && redi[j] < bi))) { best = redf[j]; bi = redi[j]; }
            msum += wm[j];
        }
        if (all) mass_s = msum;
        const float zs = __fmul_rn(row[bi], inv_t);
        const float lp = (zs - mx) - logf((float)((double)mass_s * (1.0 / 2147483648.0)));
        const int nf = bi == a.end_id ? 1 : 0;
        a.out_symbol[r] = bi;
        a.out_logprob[r] = lp;
        a.out_kept[r] = kept;
        a.out_finished[r] = nf;
        a.out_logprob_sum[r] = lps + lp;
        a.out_lengths[r] = len + 1;
        if (!nf && a.all_finished) *a.all_finished = 0;
    }
}

extern "C" int64_t nm_sample_lds_max_columns(void) { return SAMPLE_LDS_MAX_V; }

extern "C" int nm_sample_step(void* stream, const float* logits, int64_t ldx, int64_t rows, int64_t V,
                              float inv_temperature, int64_t top_k, float top_p, const uint32_t* salt_base,
                              uint32_t salt_step, int end_id, const int32_t* finished, const float* logprob_sum,
                              const int32_t* lengths, int32_t* out_symbol, float* out_logprob, int32_t* out_kept,
                              int32_t* out_finished, float* out_logprob_sum, int32_t* out_lengths,
                              int32_t* all_finished, void* workspace, int64_t workspace_bytes) {
    (void)workspace;
    NM_REQUIRE(logits && salt_base && finished && logprob_sum && lengths, "nm_sample_step: null input pointer");
    NM_REQUIRE(out_symbol && out_logprob && out_kept && out_finished && out_logprob_sum && out_lengths,
               "nm_sample_step: null output pointer");
    NM_REQUIRE(rows >= 0 && rows < (1ll << 31), "nm_sample_step: rows = %lld out of range", (long long)rows);
    NM_REQUIRE(V >= 1 && V < (1ll << 30), "nm_sample_step: V = %lld, need 1 <= V < 2^30", (long long)V);
    NM_REQUIRE(ldx >= V, "nm_sample_step: ldx = %lld < V = %lld", (long long)ldx, (long long)V);
    NM_REQUIRE(top_k >= 0, "nm_sample_step: top_k = %lld, need >= 0 (0: off)", (long long)top_k);
    NM_REQUIRE(top_p > 0.0f && top_p <= 1.0f, "nm_sample_step: top_p = %g, need 0 < top_p <= 1 (1: off)", (double)top_p);
    NM_REQUIRE(inv_temperature > 0.0f && inv_temperature <= 3.402823466e38f,
               "nm_sample_step: inv_temperature = %g, need positive and finite", (double)inv_temperature);
    NM_REQUIRE(workspace_bytes >= 0, "nm_sample_step: negative workspace_bytes");
    if (rows == 0) return NM_OK;
    SampleArgs a;
    a.x = logits; a.ldx = (long)ldx; a.V = (int)V; a.inv_t = inv_temperature;
    a.top_k = (top_k >= 1 && top_k < V) ? (int)top_k : 0;
    a.top_p = top_p;
    a.salt_base = salt_base; a.salt_step = salt_step; a.end_id = end_id;
    a.finished = finished; a.logprob_sum = logprob_sum; a.lengths = lengths;
    a.out_symbol = out_symbol; a.out_logprob = out_logprob; a.out_kept = out_kept; a.out_finished = out_finished;
    a.out_logprob_sum = out_logprob_sum; a.out_lengths = out_lengths; a.all_finished = all_finished;
    if (V <= SAMPLE_LDS_MAX_V) {
        const size_t lds = (size_t)((V * 4 + 15) / 16 * 16);
        if (lds > 48 * 1024 &&
            hipFuncSetAttribute((const void*)sample_step_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds) != hipSuccess) {
            (void)hipGetLastError();
            NM_FAIL(NM_ERR_HIP, "nm_sample_step: cannot reserve %zu bytes of LDS", lds);
        }
        hipLaunchKernelGGL(sample_step_kernel<true>, dim3((unsigned)rows), dim3(SAMPLE_NT), lds, nm_stream(stream), a);
    } else {
        hipLaunchKernelGGL(sample_step_kernel<false>, dim3((unsigned)rows), dim3(SAMPLE_NT), 0, nm_stream(stream), a);
    }
    NM_LAUNCH_CHECK("nm_sample_step");
}
