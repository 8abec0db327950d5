// Sentence-level heads (include/nmhip_pool.h): the reductions over time of encoders/pooling.py and
// encoders/attentive.py and the squared error of decoders/sequence_regressor.py.
//
//   pool_fwd_kernel<VEC, MODE>   one workgroup of 64 x 4 threads per (sentence, 256 columns): a thread owns 4 adjacent
//                                columns (one 16-byte load per position where D, ldx and the base allow; a scalar path
//                                otherwise), the 4 waves split T and combine in LDS in the fixed order 0, 1, 2, 3.  Max
//                                carries (maximum, number of positions equal to it); average carries the sum and the
//                                sentence length.  [128, 50, 1024] is 512 workgroups, 8 waves per compute unit.
//   pool_bwd_kernel<VEC, MODE>   the same decomposition; the length of an averaged sentence is one wave reduction of
//                                its mask row.  Every (b, t, d) is written.
//   time_softmax_*_kernel<HB>    one workgroup of 256 threads per (sentence, HB heads): thread i owns head i % HB and
//                                the positions i / HB, i / HB + 256 / HB, ... -- the heads are the contiguous axis, so
//                                a wave reads whole rows of energies; the reductions over T are LDS trees of fixed shape.
//   sqerr_rows_kernel            one thread per row.
//   split_mask_kernel            (include/nmhip_split.h) mask and lengths of model/sequence_split.py's longer sequence: one
//                                wavefront per sentence.
// No floating-point atomics anywhere: two runs are bit-equal.
#include "nm_common.h"

namespace {

constexpr int POOL_WAVES = 4;                // waves of a workgroup, splitting T
constexpr int POOL_COLS = 64 * 4;            // columns of a workgroup
constexpr int MODE_MAX = 0, MODE_AVG = 1;
constexpr float POOL_PAD = 1e-15f;           // pooling.py:50
constexpr float POOL_EPS = 1e-8f;            // pooling.py:63, attentive.py:73

template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ p, long d0, long D, float (&v)[4]) {
    if (VEC) {
        const float4 q = *reinterpret_cast<const float4*>(p + d0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = d0 + j < D ? p[d0 + j] : 0.0f;
    }
}
template <bool VEC>
__device__ __forceinline__ void load4i(const int32_t* __restrict__ p, long d0, long D, int (&v)[4]) {
    if (VEC) {
        const int4 q = *reinterpret_cast<const int4*>(p + d0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = d0 + j < D ? p[d0 + j] : 1;
    }
}
template <bool VEC, typename T4, typename T>
__device__ __forceinline__ void store4(T* p, long d0, long D, const T (&v)[4]) {
    if (VEC) {
        T4 q; q.x = v[0]; q.y = v[1]; q.z = v[2]; q.w = v[3];
        *reinterpret_cast<T4*>(p + d0) = q;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (d0 + j < D) p[d0 + j] = v[j];
    }
}

// p of pooling.py:50 for a 0/1 mask, as written there (x*m is exact for m in {0, 1}, whatever the contraction)
__device__ __forceinline__ float pool_padded(float x, float m) { return __fadd_rn(__fmul_rn(x, m), POOL_PAD * (1.0f - m)); }

template <bool VEC, int MODE>
__global__ __launch_bounds__(64 * POOL_WAVES) void pool_fwd_kernel(
    const float* __restrict__ x, long ldx, const float* __restrict__ mask, int T, long D, int nd, float* __restrict__ out,
    long ldo, int32_t* __restrict__ ties) {
    __shared__ float sv[POOL_WAVES][64][4];
    __shared__ int sc[POOL_WAVES][64][4];
    __shared__ float sl[POOL_WAVES];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const long b = blockIdx.x / nd;
    const long d0 = ((long)(blockIdx.x % nd) * 64 + tx) * 4;
    const bool live = d0 < D;
    const float* mb = mask + b * T;
    float v[4];
    int c[4] = {0, 0, 0, 0};
    float len = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = MODE == MODE_MAX ? -INFINITY : 0.0f;
    if (live) {
        const float* xb = x + b * T * ldx;
#pragma unroll 4
        for (int t = ty; t < T; t += POOL_WAVES) {
            const float m = mb[t];
            float xv[4];
            load4<VEC>(xb + (long)t * ldx, d0, D, xv);
            len += m;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (MODE == MODE_MAX) {
                    const float p = pool_padded(xv[j], m);
                    if (p > v[j]) { v[j] = p; c[j] = 1; }
                    else if (p == v[j]) ++c[j];
                } else {
                    v[j] += xv[j] * m;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { sv[ty][tx][j] = v[j]; sc[ty][tx][j] = c[j]; }
    if (tx == 0) sl[ty] = len;
    __syncthreads();
    if (ty != 0 || !live) return;
    len = sl[0];
    for (int w = 1; w < POOL_WAVES; ++w) {                            // fixed order: bit-equal from run to run
        len += sl[w];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float ov = sv[w][tx][j];
            const int oc = sc[w][tx][j];
            if (MODE == MODE_MAX) {
                if (ov > v[j]) { v[j] = ov; c[j] = oc; }
                else if (ov == v[j]) c[j] += oc;
            } else {
                v[j] += ov;
            }
        }
    }
    if (MODE == MODE_AVG) {
        const float den = len + POOL_EPS;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = v[j] / den;
    }
    store4<VEC, float4, float>(out + b * ldo, d0, D, v);
    if (MODE == MODE_MAX) store4<VEC, int4, int32_t>(ties + b * D, d0, D, c);
}

template <bool VEC, int MODE>
__global__ __launch_bounds__(64 * POOL_WAVES) void pool_bwd_kernel(
    const float* __restrict__ x, long ldx, const float* __restrict__ mask, const float* __restrict__ out, long ldo,
    const int32_t* __restrict__ ties, const float* __restrict__ dout, long lddo, int T, long D, int nd, float* __restrict__ dx,
    long lddx, int accumulate) {
    const int tx = threadIdx.x, ty = threadIdx.y;
    const long b = blockIdx.x / nd;
    const long d0 = ((long)(blockIdx.x % nd) * 64 + tx) * 4;
    const float* mb = mask + b * T;
    float g[4], o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (MODE == MODE_AVG) {                                          // all 64 lanes of every wave take part
        float len = 0.0f;
        for (int t = tx; t < T; t += 64) len += mb[t];
        len = nm_wave_sum(len);                                      // a sum of 0/1: exact in any order
        if (d0 >= D) return;
        load4<VEC>(dout + b * lddo, d0, D, g);
        const float den = len + POOL_EPS;
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = g[j] / den;
    } else {
        if (d0 >= D) return;
        int n[4];
        load4<VEC>(dout + b * lddo, d0, D, g);
        load4<VEC>(out + b * ldo, d0, D, o);
        load4i<VEC>(ties + b * D, d0, D, n);
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = n[j] > 1 ? g[j] / (float)n[j] : g[j];
    }
    const float* xb = MODE == MODE_MAX ? x + b * T * ldx : nullptr;
    float* dxb = dx + b * T * lddx;
#pragma unroll 2
    for (int t = ty; t < T; t += POOL_WAVES) {
        const float m = mb[t];
        float r[4];
        if (MODE == MODE_MAX) {
            float xv[4];
            load4<VEC>(xb + (long)t * ldx, d0, D, xv);
#pragma unroll
            for (int j = 0; j < 4; ++j) r[j] = (m != 0.0f && pool_padded(xv[j], m) == o[j]) ? g[j] : 0.0f;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) r[j] = m != 0.0f ? m * g[j] : 0.0f;
        }
        float* row = dxb + (long)t * lddx;
        if (accumulate) {
            float old[4];
            load4<VEC>(row, d0, D, old);
#pragma unroll
            for (int j = 0; j < 4; ++j) r[j] += old[j];
        }
        store4<VEC, float4, float>(row, d0, D, r);
    }
}

// ---- softmax over time of [B, T, H] energies ---------------------------------------------------------------------------
constexpr int TS_THREADS = 256;

template <int HB, bool IS_MAX>
__device__ __forceinline__ float ts_reduce(float* red, float v, int tid) {
    constexpr int NT = TS_THREADS / HB;
    const int tg = tid / HB;
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = NT / 2; s > 0; s >>= 1) {                            // a tree of fixed shape over the position groups
        if (tg < s) {
            const float o = red[tid + s * HB];
            red[tid] = IS_MAX ? fmaxf(red[tid], o) : red[tid] + o;
        }
        __syncthreads();
    }
    const float r = red[tid % HB];
    __syncthreads();
    return r;
}

template <int HB>
__global__ __launch_bounds__(TS_THREADS) void time_softmax_fwd_kernel(
    const float* e, long lde, const float* __restrict__ mask, int T, int H, float* w, long ldw, float* __restrict__ s_out,
    long lds, float* __restrict__ z_out) {
    constexpr int NT = TS_THREADS / HB;
    __shared__ float red[TS_THREADS];
    const int tid = threadIdx.x, hl = tid % HB, tg = tid / HB;
    const long b = blockIdx.x;
    const int h = blockIdx.y * HB + hl;
    const bool live = h < H;
    const float* eb = e + b * T * lde + h;
    const float* mb = mask != nullptr ? mask + b * T : nullptr;
    float mx = -INFINITY;
    if (live)
        for (int t = tg; t < T; t += NT) mx = fmaxf(mx, eb[(long)t * lde]);
    mx = ts_reduce<HB, true>(red, mx, tid);
    float a = 0.0f;
    if (live)
        for (int t = tg; t < T; t += NT) a += expf(eb[(long)t * lde] - mx);
    a = ts_reduce<HB, false>(red, a, tid);
    float zs = 1.0f;
    if (mb != nullptr) {                                             // (block-uniform)
        // Z = sum_t s*m + 1e-8 with s = ex / a
        float u = 0.0f;
        if (live)
            for (int t = tg; t < T; t += NT) u += (expf(eb[(long)t * lde] - mx) / a) * mb[t];
        zs = ts_reduce<HB, false>(red, u, tid) + POOL_EPS;
    }
    if (!live) return;
    if (z_out != nullptr && tg == 0) z_out[b * H + h] = zs;
    for (int t = tg; t < T; t += NT) {
        const float s = expf(eb[(long)t * lde] - mx) / a;            // (read before w, which may be e, is written)
        if (s_out != nullptr) s_out[(b * T + t) * lds + h] = s;
        w[(b * T + t) * ldw + h] = mb != nullptr ? (s * mb[t]) / zs : s;
    }
}

template <int HB>
__global__ __launch_bounds__(TS_THREADS) void time_softmax_bwd_kernel(
    const float* dw, long lddw, const float* __restrict__ s, long lds, const float* __restrict__ z,
    const float* __restrict__ mask, int T, int H, float* de, long ldde, int accumulate) {
    constexpr int NT = TS_THREADS / HB;
    __shared__ float red[TS_THREADS];
    const int tid = threadIdx.x, hl = tid % HB, tg = tid / HB;
    const long b = blockIdx.x;
    const int h = blockIdx.y * HB + hl;
    const bool live = h < H;
    const float* dwb = dw + b * T * lddw + h;
    const float* sb = s + b * T * lds + h;
    const float* mb = mask != nullptr ? mask + b * T : nullptr;
    float zs = 1.0f, r1 = 0.0f;
    if (mb != nullptr) {
        if (live) {
            zs = z[b * H + h];
            for (int t = tg; t < T; t += NT) r1 += dwb[(long)t * lddw] * (sb[(long)t * lds] * mb[t]);
        }
        r1 = ts_reduce<HB, false>(red, r1, tid);
    }
    const float shift = r1 / (zs * zs);
    float r2 = 0.0f;
    if (live)
        for (int t = tg; t < T; t += NT) {
            const float g = dwb[(long)t * lddw];
            const float ds = mb != nullptr ? (g / zs - shift) * mb[t] : g;
            r2 += ds * sb[(long)t * lds];
        }
    r2 = ts_reduce<HB, false>(red, r2, tid);
    if (!live) return;
    for (int t = tg; t < T; t += NT) {
        const float g = dwb[(long)t * lddw];
        const float ds = mb != nullptr ? (g / zs - shift) * mb[t] : g;
        float r = sb[(long)t * lds] * (ds - r2);
        float* o = de + (b * T + t) * ldde + h;
        if (accumulate) r += *o;
        *o = r;
    }
}

__global__ __launch_bounds__(256) void sqerr_rows_kernel(float* p, long ld, long rows, int dim,
                                                         const float* __restrict__ y, const float* __restrict__ grad_scale,
                                                         int write_grad, float* __restrict__ loss_rows) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const float yr = y[r];
    const float sc = 2.0f * (grad_scale != nullptr ? grad_scale[0] : 1.0f);
    float* pr = p + r * ld;
    float acc = 0.0f;
    for (int k = 0; k < dim; ++k) {
        const float d = pr[k] - yr;
        acc += d * d;
        if (write_grad) pr[k] = sc * d;
    }
    if (loss_rows != nullptr) loss_rows[r] = acc;
}

// One wavefront per sentence: lane i owns the positions i, i + 64, ...; each writes its mask entry `factor` times and the
// wave sums the row (0/1 entries: exact in fp32 below 2^24 positions, which the entry point requires).
__global__ __launch_bounds__(64) void split_mask_kernel(const float* __restrict__ mask, int T, int factor,
                                                        float* __restrict__ out_mask, int32_t* __restrict__ lengths) {
    const long b = blockIdx.x;
    const float* row = mask + b * T;
    float* out = out_mask + b * (long)T * factor;
    float sum = 0.0f;
    for (int t = threadIdx.x; t < T; t += 64) {
        const float m = row[t];
        sum += m;
        for (int j = 0; j < factor; ++j) out[(long)t * factor + j] = m;
    }
    sum = nm_wave_sum(sum);
    if (threadIdx.x == 0) lengths[b] = (int32_t)sum * factor;
}

bool pool_vec_ok(int64_t D, std::initializer_list<int64_t> lds, std::initializer_list<const void*> ptrs) {
    if (D % 4 != 0) return false;
    for (int64_t ld : lds)
        if (ld % 4 != 0) return false;
    for (const void* p : ptrs)
        if (p != nullptr && !nm_aligned16(p)) return false;
    return true;
}

int pool_check(const char* who, int mode, int64_t B, int64_t T, int64_t D) {
    NM_REQUIRE(mode == MODE_MAX || mode == MODE_AVG, "%s: mode %d is neither NM_POOL_MAX nor NM_POOL_AVG", who, mode);
    NM_REQUIRE(B >= 1 && T >= 1 && D >= 1, "%s: bad sizes B %lld, T %lld, D %lld", who, (long long)B, (long long)T,
               (long long)D);
    NM_REQUIRE(B * T < (1ll << 31) && T < (1ll << 31) - POOL_WAVES, "%s: B*T = %lld rows beyond 2^31", who,
               (long long)(B * T));
    NM_REQUIRE(B * ((D + POOL_COLS - 1) / POOL_COLS) < (1ll << 31), "%s: grid of %lld x %lld workgroups beyond 2^31", who,
               (long long)B, (long long)((D + POOL_COLS - 1) / POOL_COLS));
    return NM_OK;
}

}  // namespace

extern "C" {

int nm_pool_fwd(void* stream, int mode, const float* x, int64_t ldx, const float* mask, int64_t B, int64_t T, int64_t D,
                float* out, int64_t ldo, int32_t* ties) {
    if (int rc = pool_check("nm_pool_fwd", mode, B, T, D)) return rc;
    NM_REQUIRE(ldx >= D, "nm_pool_fwd: ldx %lld below D %lld", (long long)ldx, (long long)D);
    NM_REQUIRE(ldo >= D, "nm_pool_fwd: ldo %lld below D %lld", (long long)ldo, (long long)D);
    NM_REQUIRE(x != nullptr && mask != nullptr && out != nullptr, "nm_pool_fwd: null pointer (x, mask or out)");
    NM_REQUIRE(mode != MODE_MAX || ties != nullptr, "nm_pool_fwd: NM_POOL_MAX without ties");
    const int nd = (int)((D + POOL_COLS - 1) / POOL_COLS);
    const dim3 grid((unsigned)(B * nd)), block(64, POOL_WAVES);
    const bool vec = pool_vec_ok(D, {ldx, ldo}, {x, out, mode == MODE_MAX ? ties : nullptr});
#define NM_PF(V_, M_)                                                                                                 \
    hipLaunchKernelGGL((pool_fwd_kernel<V_, M_>), grid, block, 0, nm_stream(stream), x, (long)ldx, mask, (int)T, (long)D, \
                       nd, out, (long)ldo, ties)
    if (mode == MODE_MAX) { if (vec) NM_PF(true, MODE_MAX); else NM_PF(false, MODE_MAX); }
    else { if (vec) NM_PF(true, MODE_AVG); else NM_PF(false, MODE_AVG); }
#undef NM_PF
    NM_LAUNCH_CHECK("nm_pool_fwd");
}

int nm_pool_bwd(void* stream, int mode, const float* x, int64_t ldx, const float* mask, const float* out, int64_t ldo,
                const int32_t* ties, const float* dout, int64_t lddo, int64_t B, int64_t T, int64_t D, float* dx,
                int64_t lddx, int accumulate) {
    if (int rc = pool_check("nm_pool_bwd", mode, B, T, D)) return rc;
    NM_REQUIRE(lddo >= D, "nm_pool_bwd: lddo %lld below D %lld", (long long)lddo, (long long)D);
    NM_REQUIRE(lddx >= D, "nm_pool_bwd: lddx %lld below D %lld", (long long)lddx, (long long)D);
    NM_REQUIRE(mask != nullptr && dout != nullptr && dx != nullptr, "nm_pool_bwd: null pointer (mask, dout or dx)");
    if (mode == MODE_MAX) {
        NM_REQUIRE(ldx >= D, "nm_pool_bwd: ldx %lld below D %lld", (long long)ldx, (long long)D);
        NM_REQUIRE(ldo >= D, "nm_pool_bwd: ldo %lld below D %lld", (long long)ldo, (long long)D);
        NM_REQUIRE(x != nullptr && out != nullptr && ties != nullptr,
                   "nm_pool_bwd: NM_POOL_MAX without x, out or ties of the forward call");
        const float* x_end = x + (B * T - 1) * ldx + D;
        const float* dx_end = dx + (B * T - 1) * lddx + D;
        NM_REQUIRE(dx_end <= x || x_end <= dx, "nm_pool_bwd: dx aliasing x");
    }
    const int nd = (int)((D + POOL_COLS - 1) / POOL_COLS);
    const dim3 grid((unsigned)(B * nd)), block(64, POOL_WAVES);
    const bool is_max = mode == MODE_MAX;
    const bool vec = pool_vec_ok(D, {lddo, lddx, is_max ? ldx : 0, is_max ? ldo : 0},
                                 {dout, dx, is_max ? x : nullptr, is_max ? out : nullptr, is_max ? ties : nullptr});
#define NM_PB(V_, M_)                                                                                                \
    hipLaunchKernelGGL((pool_bwd_kernel<V_, M_>), grid, block, 0, nm_stream(stream), x, (long)ldx, mask, out, (long)ldo, \
                       ties, dout, (long)lddo, (int)T, (long)D, nd, dx, (long)lddx, accumulate ? 1 : 0)
    if (is_max) { if (vec) NM_PB(true, MODE_MAX); else NM_PB(false, MODE_MAX); }
    else { if (vec) NM_PB(true, MODE_AVG); else NM_PB(false, MODE_AVG); }
#undef NM_PB
    NM_LAUNCH_CHECK("nm_pool_bwd");
}

#define NM_TS_DISPATCH(KERNEL_, ...)                                                                       \
    do {                                                                                                   \
        int hb = 1;                                                                                        \
        while (hb < 64 && hb < H) hb <<= 1;                                                                \
        const dim3 grid((unsigned)B, (unsigned)((H + hb - 1) / hb)), block(TS_THREADS);                    \
        switch (hb) {                                                                                      \
            case 1: hipLaunchKernelGGL((KERNEL_<1>), grid, block, 0, nm_stream(stream), __VA_ARGS__); break;   \
            case 2: hipLaunchKernelGGL((KERNEL_<2>), grid, block, 0, nm_stream(stream), __VA_ARGS__); break;   \
            case 4: hipLaunchKernelGGL((KERNEL_<4>), grid, block, 0, nm_stream(stream), __VA_ARGS__); break;   \
            case 8: hipLaunchKernelGGL((KERNEL_<8>), grid, block, 0, nm_stream(stream), __VA_ARGS__); break;   \
            case 16: hipLaunchKernelGGL((KERNEL_<16>), grid, block, 0, nm_stream(stream), __VA_ARGS__); break; \
            case 32: hipLaunchKernelGGL((KERNEL_<32>), grid, block, 0, nm_stream(stream), __VA_ARGS__); break; \
            default: hipLaunchKernelGGL((KERNEL_<64>), grid, block, 0, nm_stream(stream), __VA_ARGS__); break; \
        }                                                                                                  \
    } while (0)

static int time_softmax_check(const char* who, int64_t B, int64_t T, int64_t H) {
    NM_REQUIRE(B >= 1 && T >= 1 && H >= 1, "%s: bad sizes B %lld, T %lld, H %lld", who, (long long)B, (long long)T,
               (long long)H);
    NM_REQUIRE(B < (1ll << 31) && T < (1ll << 31) - TS_THREADS && B * T < (1ll << 31) && H <= 64ll * NM_MAX_GRID_Y,
               "%s: sizes B %lld, T %lld, H %lld beyond the grid", who, (long long)B, (long long)T, (long long)H);
    return NM_OK;
}

int nm_time_softmax_fwd(void* stream, const float* e, int64_t lde, const float* mask, int64_t B, int64_t T, int64_t H,
                        float* w, int64_t ldw, float* s_out, int64_t lds, float* z_out) {
    if (int rc = time_softmax_check("nm_time_softmax_fwd", B, T, H)) return rc;
    NM_REQUIRE(lde >= H, "nm_time_softmax_fwd: lde %lld below H %lld", (long long)lde, (long long)H);
    NM_REQUIRE(ldw >= H, "nm_time_softmax_fwd: ldw %lld below H %lld", (long long)ldw, (long long)H);
    NM_REQUIRE(s_out == nullptr || lds >= H, "nm_time_softmax_fwd: lds %lld below H %lld", (long long)lds, (long long)H);
    NM_REQUIRE(e != nullptr && w != nullptr, "nm_time_softmax_fwd: null pointer (e or w)");
    NM_TS_DISPATCH(time_softmax_fwd_kernel, e, (long)lde, mask, (int)T, (int)H, w, (long)ldw, s_out, (long)lds, z_out);
    NM_LAUNCH_CHECK("nm_time_softmax_fwd");
}

int nm_time_softmax_bwd(void* stream, const float* dw, int64_t lddw, const float* s, int64_t lds, const float* z,
                        const float* mask, int64_t B, int64_t T, int64_t H, float* de, int64_t ldde, int accumulate) {
    if (int rc = time_softmax_check("nm_time_softmax_bwd", B, T, H)) return rc;
    NM_REQUIRE(lddw >= H, "nm_time_softmax_bwd: lddw %lld below H %lld", (long long)lddw, (long long)H);
    NM_REQUIRE(lds >= H, "nm_time_softmax_bwd: lds %lld below H %lld", (long long)lds, (long long)H);
    NM_REQUIRE(ldde >= H, "nm_time_softmax_bwd: ldde %lld below H %lld", (long long)ldde, (long long)H);
    NM_REQUIRE(dw != nullptr && s != nullptr && de != nullptr, "nm_time_softmax_bwd: null pointer (dw, s or de)");
    NM_REQUIRE(mask == nullptr || z != nullptr, "nm_time_softmax_bwd: mask without z");
    NM_REQUIRE(!(accumulate && de == dw), "nm_time_softmax_bwd: accumulate into dw itself");
    NM_TS_DISPATCH(time_softmax_bwd_kernel, dw, (long)lddw, s, (long)lds, z, mask, (int)T, (int)H, de, (long)ldde,
                   accumulate ? 1 : 0);
    NM_LAUNCH_CHECK("nm_time_softmax_bwd");
}

int nm_sqerr_rows(void* stream, float* pred, int64_t ld, int64_t rows, int64_t dim, const float* targets,
                  const float* grad_scale, int write_grad, float* loss_rows) {
    NM_REQUIRE(dim >= 1 && dim < (1ll << 31), "nm_sqerr_rows: dimension %lld, at least 1 is needed", (long long)dim);
    NM_REQUIRE(rows >= 0 && rows < (1ll << 31) - 256, "nm_sqerr_rows: bad row count %lld", (long long)rows);
    NM_REQUIRE(ld >= dim, "nm_sqerr_rows: ld %lld below the dimension %lld", (long long)ld, (long long)dim);
    if (rows == 0) return NM_OK;
    NM_REQUIRE(pred != nullptr && targets != nullptr, "nm_sqerr_rows: null pointer (pred or targets)");
    hipLaunchKernelGGL(sqerr_rows_kernel, dim3((unsigned)nm_cdiv(rows, 256)), dim3(256), 0, nm_stream(stream), pred,
                       (long)ld, (long)rows, (int)dim, targets, grad_scale, write_grad ? 1 : 0, loss_rows);
    NM_LAUNCH_CHECK("nm_sqerr_rows");
}

// include/nmhip_split.h
int nm_split_mask(void* stream, const float* mask, int64_t B, int64_t T, int64_t factor, float* out_mask,
                  int32_t* lengths) {
    NM_REQUIRE(B >= 1 && T >= 1 && factor >= 1, "nm_split_mask: bad sizes B %lld, T %lld, factor %lld", (long long)B,
               (long long)T, (long long)factor);
    NM_REQUIRE(B < (1ll << 31) && T < (1ll << 24) && factor < (1ll << 24) && T * factor < (1ll << 31),
               "nm_split_mask: sizes B %lld, T %lld, factor %lld beyond the grid or the exact fp32 row sum", (long long)B,
               (long long)T, (long long)factor);
    NM_REQUIRE(mask != nullptr && out_mask != nullptr && lengths != nullptr,
               "nm_split_mask: null pointer (mask, out_mask or lengths)");
    const float* in_end = mask + B * T;
    const float* out_end = out_mask + B * T * factor;
    NM_REQUIRE(out_end <= mask || in_end <= out_mask, "nm_split_mask: out_mask aliasing mask");
    hipLaunchKernelGGL(split_mask_kernel, dim3((unsigned)B), dim3(64), 0, nm_stream(stream), mask, (int)T, (int)factor,
                       out_mask, lengths);
    NM_LAUNCH_CHECK("nm_split_mask");
}

}  // extern "C"
