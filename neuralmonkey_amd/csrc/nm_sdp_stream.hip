// libnmhip: multi-head scaled dot-product attention over sequences that do not fit LDS (include/nmhip_sdp_stream.h,
// DESIGN 4.21).  The resident kernels (nm_sdp_attention.hip, nm_sdp_mfma.hip) keep the whole key / value tile of a head
// in LDS and save the [Bq, H, Tq, Tk] softmax output for the backward pass; these stream tiles of 64 positions through a
// two-stage LDS ring, carry the softmax online (running maximum and sum in registers) and, backward, recompute the
// weights from the saved row maximum and row sum.  Same arithmetic (nm_sdp.h), fp32 on v_mfma_f32_16x16x4_f32, the
// transposed formulation of nm_sdp_mfma.hip: the accumulators of one product are the B operand of the next, so neither
// the weights nor the energy gradients leave the registers.
//
//     A: lane l holds A[m = l & 15][k = l >> 4]      B: lane l holds B[k = l >> 4][n = l & 15]
//     D: lane l, register r holds D[m = 4 (l >> 4) + r][n = l & 15]
//
//   forward, dQ     a workgroup = (b, h, 64 queries), a wave owns 16 queries i (n = i); per key tile
//       S^T[j][i] = sum_c K[j][c] Qs[i][c]            A = K tile (LDS, 16-byte reads along c), B = scaled queries (regs)
//       forward:  P = exp(e - m_new), the context accumulators and the sum rescaled by exp(m_old - m_new): in this
//                 layout every accumulator of a lane belongs to ONE query, so the rescale is one scalar per lane
//                 C^T[c][i] += sum_j V[j][c] Pd[i][j]  A = V tile (LDS, by rows), B = the S^T accumulators
//       dQ:       dW^T[j][i] = sum_c V[j][c] dO[i][c] ; dE = P (dW keep - D) ; dQ^T[c][i] += sum_j K[j][c] dE[i][j]
//   dK / dV         a workgroup = (b, h, 64 keys), a wave owns 16 keys j (n = j), K and V rows in registers; per query tile
//       S[i][j] = sum_c Qs[i][c] K[j][c] ; dW[i][j] = sum_c dO[i][c] V[j][c]      A = Qs / dO tile (LDS), B = registers
//       dV^T[c][j] += sum_i dO[i][c] Pd[i][j] ; dK^T[c][j] += sum_i Qs[i][c] dE[i][j]
//
// One LDS layout serves both ways a tile is read: rows of dh + 4 floats.  "By rows" (16 channels of 4 rows per
// instruction, ds_read_b32) the stride = 4 mod 8 is conflict-free as in nm_sdp_mfma.hip; "along c" a lane reads 16
// bytes of one row (ds_read_b128), and the row stride is an odd number of 16-byte units.  Tiles are written with
// 16-byte stores.  The ring: the global loads of tile t + 1 are issued into registers before the products of tile t and
// stored to the other stage after them; one barrier per tile.  Nothing here communicates between workgroups.
#include "nm_sdp.h"
#include "../../include/nmhip_sdp_stream.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define NM_MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)
#define ST_TILE 64                                   // positions per streamed tile

__device__ __forceinline__ float st_xor16(float v) { return __shfl_xor(v, 16, 64); }
__device__ __forceinline__ float st_xor32(float v) { return __shfl_xor(v, 32, 64); }

// rows row0 .. row0 + 63 of a [rows, H * dh] matrix, the head's dh columns: thread tid holds quads tid + 256 u
template <int NDT>
__device__ __forceinline__ void st_load(float4 (&r)[NDT], const float* g, int d, int row0, int rows, int tid) {
#pragma unroll
    for (int u = 0; u < NDT; ++u) {
        const int idx = tid + 256 * u;
        const int j = idx / (4 * NDT), c = (idx - j * (4 * NDT)) * 4;
        r[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row0 + j < rows) r[u] = *reinterpret_cast<const float4*>(g + (long)(row0 + j) * d + c);
    }
}

template <int NDT>
__device__ __forceinline__ void st_store(float* tile, const float4 (&r)[NDT], int tid, float scale) {
    constexpr int LD = 16 * NDT + 4;
#pragma unroll
    for (int u = 0; u < NDT; ++u) {
        const int idx = tid + 256 * u;
        const int j = idx / (4 * NDT), c = (idx - j * (4 * NDT)) * 4;
        *reinterpret_cast<float4*>(tile + j * LD + c) =
            make_float4(r[u].x * scale, r[u].y * scale, r[u].z * scale, r[u].w * scale);
    }
}

// acc[tt][r] = sum_c tile[16 tt + 4 g + r][c] * B[c][n]: the tile's rows are the m index, bf the lane's dh / 4 channels
template <int NDT>
__device__ __forceinline__ void st_scores(f32x4 (&acc)[4], const float* tile, const float (&bf)[4 * NDT], int l15,
                                          int g) {
    constexpr int LD = 16 * NDT + 4, KQ = 4 * NDT;
    const float* ar = tile + l15 * LD + g * KQ;
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) acc[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c4 = 0; c4 < NDT; ++c4) {
        float4 a[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) a[tt] = *reinterpret_cast<const float4*>(ar + tt * 16 * LD + 4 * c4);
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) acc[tt] = NM_MFMA16(a[tt].x, bf[4 * c4 + 0], acc[tt]);
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) acc[tt] = NM_MFMA16(a[tt].y, bf[4 * c4 + 1], acc[tt]);
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) acc[tt] = NM_MFMA16(a[tt].z, bf[4 * c4 + 2], acc[tt]);
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) acc[tt] = NM_MFMA16(a[tt].w, bf[4 * c4 + 3], acc[tt]);
    }
}

// out[dt][r] += sum over the tile's rows x = 16 tt + 4 g + r of tile[x][16 dt + l15] * bw[tt][r]
template <int NDT>
__device__ __forceinline__ void st_accum(f32x4 (&out)[NDT], const float* tile, const f32x4 (&bw)[4], int l15, int g) {
    constexpr int LD = 16 * NDT + 4;
#pragma unroll
    for (int tt = 0; tt < 4; ++tt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float* ar = tile + (16 * tt + 4 * g + r) * LD + l15;
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) out[dt] = NM_MFMA16(ar[16 * dt], bw[tt][r], out[dt]);
        }
}

template <int NDT>
__device__ __forceinline__ void st_load_row(float (&f)[4 * NDT], const float* row, float scale) {
#pragma unroll
    for (int c4 = 0; c4 < NDT; ++c4) {
        const float4 t = *reinterpret_cast<const float4*>(row + 4 * c4);
        f[4 * c4 + 0] = t.x * scale; f[4 * c4 + 1] = t.y * scale;
        f[4 * c4 + 2] = t.z * scale; f[4 * c4 + 3] = t.w * scale;
    }
}

// ---------------------------------------------------------------------------------------------
// forward: grid (Bq * H, ceil(Tq / 64)), 4 waves of 16 queries.  A stage = K tile, V tile, 64 mask values.
// ---------------------------------------------------------------------------------------------
template <int NDT>
__global__ __launch_bounds__(256) void sdp_stream_fwd_kernel(SdpArgs p, float* __restrict__ row_max,
                                                             float* __restrict__ row_sum) {
    constexpr int DH = 16 * NDT, KQ = 4 * NDT, LD = DH + 4, TILE = ST_TILE * LD, STAGE = 2 * TILE + ST_TILE;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const int h = blockIdx.x % p.H, b = blockIdx.x / p.H;
    const int kb = b / p.rpk;
    const int d = p.H * DH;
    const float* kg = p.k + (long)kb * p.k_bs + (long)h * DH;
    const float* vg = p.v + (long)kb * p.v_bs + (long)h * DH;
    const float* mg = p.mask ? p.mask + (long)kb * p.mask_bs : nullptr;
    const int ntile = (p.Tk + ST_TILE - 1) / ST_TILE;

    const int i0 = (int)blockIdx.y * 64 + wave * 16;
    const bool wave_on = i0 < p.Tq;                  // a wave without queries still feeds the ring
    const int i = i0 + l15;
    const bool iok = i < p.Tq;
    float qf[KQ];
    st_load_row<NDT>(qf, p.q + (long)b * p.q_bs + (long)(iok ? i : p.Tq - 1) * d + (long)h * DH + g * KQ, p.scale);

    float4 kr[NDT], vr[NDT];
    float mr = 1.0f;
    st_load<NDT>(kr, kg, d, 0, p.Tk, tid);
    st_load<NDT>(vr, vg, d, 0, p.Tk, tid);
    if (tid < ST_TILE && mg && tid < p.Tk) mr = mg[tid];
    st_store<NDT>(sm, kr, tid, 1.0f);
    st_store<NDT>(sm + TILE, vr, tid, 1.0f);
    if (tid < ST_TILE) sm[2 * TILE + tid] = mr;
    __syncthreads();

    float m = -INFINITY, l = 0.0f;                   // l: this lane's share of the row sum (reduced at the end)
    f32x4 cacc[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) cacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < ntile; ++t) {
        const float* st = sm + (t & 1) * STAGE;
        const bool more = t + 1 < ntile;
        if (more) {
            const int j1 = (t + 1) * ST_TILE;
            st_load<NDT>(kr, kg, d, j1, p.Tk, tid);
            st_load<NDT>(vr, vg, d, j1, p.Tk, tid);
            mr = 1.0f;
            if (tid < ST_TILE && mg && j1 + tid < p.Tk) mr = mg[j1 + tid];
        }
        if (wave_on) {
            f32x4 acc[4];
            st_scores<NDT>(acc, st, qf, l15, g);
            const float* ms = st + 2 * TILE;
            float tmax = -INFINITY;
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int jl = 16 * tt + 4 * g + r, j = t * ST_TILE + jl;
                    const float e = j < p.Tk ? sdp_masked_energy(p, acc[tt][r], i, j, ms[jl]) : -INFINITY;
                    acc[tt][r] = e;
                    tmax = fmaxf(tmax, e);
                }
            tmax = fmaxf(tmax, st_xor16(tmax));
            tmax = fmaxf(tmax, st_xor32(tmax));
            const float mn = fmaxf(m, tmax);         // finite: every tile holds at least one key
            const float sc = expf(m - mn);           // 0 on the first tile, and when -1e9 gives way to a real energy
            float ls = 0.0f;
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float ex = expf(acc[tt][r] - mn);
                    ls += ex;
                    acc[tt][r] = ex * sdp_keep(p, b, h, i, t * ST_TILE + 16 * tt + 4 * g + r);
                }
            l = l * sc + ls;
            m = mn;
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) {
                cacc[dt][0] *= sc; cacc[dt][1] *= sc; cacc[dt][2] *= sc; cacc[dt][3] *= sc;
            }
            st_accum<NDT>(cacc, st + TILE, acc, l15, g);
        }
        if (more) {
            float* nx = sm + ((t + 1) & 1) * STAGE;
            st_store<NDT>(nx, kr, tid, 1.0f);
            st_store<NDT>(nx + TILE, vr, tid, 1.0f);
            if (tid < ST_TILE) nx[2 * TILE + tid] = mr;
        }
        __syncthreads();
    }
    l += st_xor16(l);
    l += st_xor32(l);
    const float inv = 1.0f / l;
    if (wave_on && iok) {
        float* cg = p.ctx + (long)b * p.ctx_bs + (long)i * d + (long)h * DH + 4 * g;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
            *reinterpret_cast<float4*>(cg + 16 * dt) =
                make_float4(cacc[dt][0] * inv, cacc[dt][1] * inv, cacc[dt][2] * inv, cacc[dt][3] * inv);
        if (row_max && g == 0) {
            const long ri = ((long)b * p.H + h) * p.Tq + i;
            row_max[ri] = m;
            row_sum[ri] = l;
        }
    }
    if (!p.weights) return;                          // (uniform)

    // second sweep: the softmax output exp(e - m) / l, from the keys alone
    st_load<NDT>(kr, kg, d, 0, p.Tk, tid);
    mr = 1.0f;
    if (tid < ST_TILE && mg && tid < p.Tk) mr = mg[tid];
    st_store<NDT>(sm, kr, tid, 1.0f);
    if (tid < ST_TILE) sm[2 * TILE + tid] = mr;
    __syncthreads();
    float* wg = p.weights + (((long)b * p.H + h) * p.Tq + (iok ? i : 0)) * p.Tk;
    const bool quads = ((p.Tk & 3) == 0) && nm_aligned16_dev(p.weights);
    for (int t = 0; t < ntile; ++t) {
        const float* st = sm + (t & 1) * STAGE;
        const bool more = t + 1 < ntile;
        if (more) {
            const int j1 = (t + 1) * ST_TILE;
            st_load<NDT>(kr, kg, d, j1, p.Tk, tid);
            mr = 1.0f;
            if (tid < ST_TILE && mg && j1 + tid < p.Tk) mr = mg[j1 + tid];
        }
        if (wave_on) {
            f32x4 acc[4];
            st_scores<NDT>(acc, st, qf, l15, g);
            const float* ms = st + 2 * TILE;
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                const int jl = 16 * tt + 4 * g, j0 = t * ST_TILE + jl;
                float w[4];
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    w[r] = j0 + r < p.Tk ? expf(sdp_masked_energy(p, acc[tt][r], i, j0 + r, ms[jl + r]) - m) * inv : 0.0f;
                if (iok) {
                    if (quads) {                     // Tk a multiple of 4: a quad never straddles the row's end
                        if (j0 < p.Tk) *reinterpret_cast<float4*>(wg + j0) = make_float4(w[0], w[1], w[2], w[3]);
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (j0 + r < p.Tk) wg[j0 + r] = w[r];
                    }
                }
            }
        }
        if (more) {
            float* nx = sm + ((t + 1) & 1) * STAGE;
            st_store<NDT>(nx, kr, tid, 1.0f);
            if (tid < ST_TILE) nx[2 * TILE + tid] = mr;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// backward 1: D[b, h, i] = dctx_i . ctx_i over the head's channels (= sum_j dW_ij W_ij, also under weight dropout:
// ctx was formed from the dropped weights).  A thread per (b, i, h), channels in order.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sdp_stream_dsum_kernel(const float* __restrict__ ctx, long ctx_bs,
                                                              const float* __restrict__ dctx, long dctx_bs,
                                                              float* __restrict__ dsum, int H, int dh, int Tq,
                                                              long total) {
    for (long x = (long)blockIdx.x * 256 + threadIdx.x; x < total; x += (long)gridDim.x * 256) {
        const int h = (int)(x % H);
        const long bi = x / H;
        const int i = (int)(bi % Tq);
        const long b = bi / Tq;
        const float* c = ctx + b * ctx_bs + ((long)i * H + h) * dh;
        const float* g = dctx + b * dctx_bs + ((long)i * H + h) * dh;
        float acc = 0.0f;
        for (int c4 = 0; c4 < dh; c4 += 4) {
            const float4 u = *reinterpret_cast<const float4*>(c + c4), w = *reinterpret_cast<const float4*>(g + c4);
            acc += (u.x * w.x + u.y * w.y) + (u.z * w.z + u.w * w.w);
        }
        dsum[(b * H + h) * Tq + i] = acc;
    }
}

struct SdpStreamBwdArgs {
    SdpBwdArgs a;                                    // a.de: the D workspace [B, H, Tq]
    const float* row_max;
    const float* row_sum;
};

// ---------------------------------------------------------------------------------------------
// backward 2, dQ: grid (B * H, ceil(Tq / 64)), 4 waves of 16 queries; the key / value tiles stream as in the forward
// ---------------------------------------------------------------------------------------------
template <int NDT>
__global__ __launch_bounds__(256) void sdp_stream_dq_kernel(SdpStreamBwdArgs s) {
    constexpr int DH = 16 * NDT, KQ = 4 * NDT, LD = DH + 4, TILE = ST_TILE * LD, STAGE = 2 * TILE + ST_TILE;
    const SdpBwdArgs& a = s.a;
    const SdpArgs& p = a.f;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const int h = blockIdx.x % p.H, b = blockIdx.x / p.H;
    const int d = p.H * DH;
    const float* kg = p.k + (long)b * p.k_bs + (long)h * DH;
    const float* vg = p.v + (long)b * p.v_bs + (long)h * DH;
    const float* mg = p.mask ? p.mask + (long)b * p.mask_bs : nullptr;
    const int ntile = (p.Tk + ST_TILE - 1) / ST_TILE;

    const int i0 = (int)blockIdx.y * 64 + wave * 16;
    const bool wave_on = i0 < p.Tq;
    const int i = i0 + l15;
    const bool iok = i < p.Tq;
    const int ic = iok ? i : p.Tq - 1;
    float qf[KQ], dof[KQ];
    st_load_row<NDT>(qf, p.q + (long)b * p.q_bs + (long)ic * d + (long)h * DH + g * KQ, p.scale);
    st_load_row<NDT>(dof, a.dctx + (long)b * a.dctx_bs + (long)ic * d + (long)h * DH + g * KQ, 1.0f);
    const long ri = ((long)b * p.H + h) * p.Tq + ic;
    const float m = s.row_max[ri], inv = 1.0f / s.row_sum[ri], dsum = a.de[ri];

    float4 kr[NDT], vr[NDT];
    float mr = 1.0f;
    st_load<NDT>(kr, kg, d, 0, p.Tk, tid);
    st_load<NDT>(vr, vg, d, 0, p.Tk, tid);
    if (tid < ST_TILE && mg && tid < p.Tk) mr = mg[tid];
    st_store<NDT>(sm, kr, tid, 1.0f);
    st_store<NDT>(sm + TILE, vr, tid, 1.0f);
    if (tid < ST_TILE) sm[2 * TILE + tid] = mr;
    __syncthreads();

    f32x4 qacc[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) qacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < ntile; ++t) {
        const float* st = sm + (t & 1) * STAGE;
        const bool more = t + 1 < ntile;
        if (more) {
            const int j1 = (t + 1) * ST_TILE;
            st_load<NDT>(kr, kg, d, j1, p.Tk, tid);
            st_load<NDT>(vr, vg, d, j1, p.Tk, tid);
            mr = 1.0f;
            if (tid < ST_TILE && mg && j1 + tid < p.Tk) mr = mg[j1 + tid];
        }
        if (wave_on) {
            f32x4 acc[4], dw[4];
            st_scores<NDT>(acc, st, qf, l15, g);
            st_scores<NDT>(dw, st + TILE, dof, l15, g);
            const float* ms = st + 2 * TILE;
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int jl = 16 * tt + 4 * g + r, j = t * ST_TILE + jl;
                    const float mk = ms[jl];
                    const float e = j < p.Tk ? sdp_masked_energy(p, acc[tt][r], i, j, mk) : -INFINITY;
                    const float w = expf(e - m) * inv;                      // the forward's weight, recomputed
                    float de = w * (dw[tt][r] * sdp_keep(p, b, h, i, j) - dsum);
                    if (p.causal && j > i + p.Tk - p.Tq) de = 0.0f;         // tf.where passes no gradient
                    de *= mk;                                               // e*m + const
                    acc[tt][r] = de;
                }
            st_accum<NDT>(qacc, st, acc, l15, g);
        }
        if (more) {
            float* nx = sm + ((t + 1) & 1) * STAGE;
            st_store<NDT>(nx, kr, tid, 1.0f);
            st_store<NDT>(nx + TILE, vr, tid, 1.0f);
            if (tid < ST_TILE) nx[2 * TILE + tid] = mr;
        }
        __syncthreads();
    }
    if (wave_on && iok) {
        float* dqg = a.dq + (long)b * a.dq_bs + (long)i * d + (long)h * DH + 4 * g;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
            float4 o = make_float4(qacc[dt][0] * p.scale, qacc[dt][1] * p.scale, qacc[dt][2] * p.scale,
                                   qacc[dt][3] * p.scale);
            float4* dst = reinterpret_cast<float4*>(dqg + 16 * dt);
            if (a.accumulate) {
                const float4 old = *dst;
                o.x += old.x; o.y += old.y; o.z += old.z; o.w += old.w;
            }
            *dst = o;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// backward 3, dK / dV: grid (B * H, ceil(Tk / 64)), 4 waves of 16 keys whose K and V rows stay in registers.  A stage
// = scaled-Q tile, dctx tile, and per query of the tile the row maximum, 1 / row sum and D.
// ---------------------------------------------------------------------------------------------
template <int NDT>
__global__ __launch_bounds__(256) void sdp_stream_dkv_kernel(SdpStreamBwdArgs s) {
    constexpr int DH = 16 * NDT, KQ = 4 * NDT, LD = DH + 4, TILE = ST_TILE * LD, STAGE = 2 * TILE + 3 * ST_TILE;
    const SdpBwdArgs& a = s.a;
    const SdpArgs& p = a.f;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const int h = blockIdx.x % p.H, b = blockIdx.x / p.H;
    const int d = p.H * DH;
    const float* qg = p.q + (long)b * p.q_bs + (long)h * DH;
    const float* gg = a.dctx + (long)b * a.dctx_bs + (long)h * DH;
    const long rbase = ((long)b * p.H + h) * p.Tq;
    const int ntile = (p.Tq + ST_TILE - 1) / ST_TILE;

    const int j0 = (int)blockIdx.y * 64 + wave * 16;
    const bool wave_on = j0 < p.Tk;
    const int j = j0 + l15;
    const bool jok = j < p.Tk;
    const int jc = jok ? j : p.Tk - 1;
    float kf[KQ], vf[KQ];
    st_load_row<NDT>(kf, p.k + (long)b * p.k_bs + (long)jc * d + (long)h * DH + g * KQ, 1.0f);
    st_load_row<NDT>(vf, p.v + (long)b * p.v_bs + (long)jc * d + (long)h * DH + g * KQ, 1.0f);
    const float mk = p.mask ? p.mask[(long)b * p.mask_bs + jc] : 1.0f;

    // per-query statistics of a tile: threads 0..63 the maximum, 64..127 1 / sum, 128..191 D
    const int swhich = tid >> 6, sl = tid & 63;
    auto stat = [&](int q0) -> float {
        if (swhich > 2 || q0 + sl >= p.Tq) return swhich == 1 ? 1.0f : 0.0f;
        const long x = rbase + q0 + sl;
        return swhich == 0 ? s.row_max[x] : swhich == 1 ? 1.0f / s.row_sum[x] : a.de[x];
    };
    float4 qr[NDT], gr[NDT];
    st_load<NDT>(qr, qg, d, 0, p.Tq, tid);
    st_load<NDT>(gr, gg, d, 0, p.Tq, tid);
    float sr = stat(0);
    st_store<NDT>(sm, qr, tid, p.scale);
    st_store<NDT>(sm + TILE, gr, tid, 1.0f);
    if (tid < 3 * ST_TILE) sm[2 * TILE + tid] = sr;
    __syncthreads();

    f32x4 dk[NDT], dv[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
        dk[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int t = 0; t < ntile; ++t) {
        const float* st = sm + (t & 1) * STAGE;
        const bool more = t + 1 < ntile;
        if (more) {
            st_load<NDT>(qr, qg, d, (t + 1) * ST_TILE, p.Tq, tid);
            st_load<NDT>(gr, gg, d, (t + 1) * ST_TILE, p.Tq, tid);
            sr = stat((t + 1) * ST_TILE);
        }
        if (wave_on) {
            f32x4 acc[4], dw[4];
            st_scores<NDT>(acc, st, kf, l15, g);
            st_scores<NDT>(dw, st + TILE, vf, l15, g);
            const float* ss = st + 2 * TILE;
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int il = 16 * tt + 4 * g + r, i = t * ST_TILE + il;
                    const float e = sdp_masked_energy(p, acc[tt][r], i, j, mk);
                    const float w = i < p.Tq ? expf(e - ss[il]) * ss[ST_TILE + il] : 0.0f;
                    const float keep = sdp_keep(p, b, h, i, j);
                    float de = w * (dw[tt][r] * keep - ss[2 * ST_TILE + il]);
                    if (p.causal && j > i + p.Tk - p.Tq) de = 0.0f;
                    de *= mk;
                    acc[tt][r] = de;
                    dw[tt][r] = w * keep;
                }
            st_accum<NDT>(dk, st, acc, l15, g);
            st_accum<NDT>(dv, st + TILE, dw, l15, g);
        }
        if (more) {
            float* nx = sm + ((t + 1) & 1) * STAGE;
            st_store<NDT>(nx, qr, tid, p.scale);
            st_store<NDT>(nx + TILE, gr, tid, 1.0f);
            if (tid < 3 * ST_TILE) nx[2 * TILE + tid] = sr;
        }
        __syncthreads();
    }
    if (wave_on && jok) {
        float* dkg = a.dk + (long)b * a.dk_bs + (long)j * d + (long)h * DH + 4 * g;
        float* dvg = a.dv + (long)b * a.dv_bs + (long)j * d + (long)h * DH + 4 * g;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
            float4 ok = make_float4(dk[dt][0], dk[dt][1], dk[dt][2], dk[dt][3]);
            float4 ov = make_float4(dv[dt][0], dv[dt][1], dv[dt][2], dv[dt][3]);
            float4* pk = reinterpret_cast<float4*>(dkg + 16 * dt);
            float4* pv = reinterpret_cast<float4*>(dvg + 16 * dt);
            if (a.accumulate) {
                const float4 a0 = *pk, a1 = *pv;
                ok.x += a0.x; ok.y += a0.y; ok.z += a0.z; ok.w += a0.w;
                ov.x += a1.x; ov.y += a1.y; ov.z += a1.z; ov.w += a1.w;
            }
            *pk = ok;
            *pv = ov;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
static size_t st_lds(long dh, int extra) { return sizeof(float) * 2 * (2 * ST_TILE * (dh + 4) + extra * ST_TILE); }

// the attribute is per DEVICE (library contexts exist per device: nm_create): one bit per device id
template <typename K>
static void st_allow_lds(K kernel, std::atomic<unsigned>& devs, size_t lds) {
    const unsigned bit = 1u << (nm_cur()->device & 31);
    if (devs.load(std::memory_order_relaxed) & bit) return;
    (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    devs.fetch_or(bit, std::memory_order_relaxed);
}

template <int NDT>
static void st_launch_fwd(const SdpArgs& p, float* row_max, float* row_sum, hipStream_t st) {
    static std::atomic<unsigned> devs{0};
    const size_t lds = st_lds(16 * NDT, 1);
    st_allow_lds(sdp_stream_fwd_kernel<NDT>, devs, lds);
    hipLaunchKernelGGL((sdp_stream_fwd_kernel<NDT>), dim3((unsigned)(p.Bq * p.H), (unsigned)((p.Tq + 63) / 64)),
                       dim3(256), lds, st, p, row_max, row_sum);
}

template <int NDT>
static void st_launch_bwd(const SdpStreamBwdArgs& s, hipStream_t st) {
    static std::atomic<unsigned> devs_q{0}, devs_kv{0};
    const SdpArgs& p = s.a.f;
    const size_t lds_q = st_lds(16 * NDT, 1), lds_kv = st_lds(16 * NDT, 3);
    st_allow_lds(sdp_stream_dq_kernel<NDT>, devs_q, lds_q);
    st_allow_lds(sdp_stream_dkv_kernel<NDT>, devs_kv, lds_kv);
    hipLaunchKernelGGL((sdp_stream_dq_kernel<NDT>), dim3((unsigned)(p.Bq * p.H), (unsigned)((p.Tq + 63) / 64)),
                       dim3(256), lds_q, st, s);
    hipLaunchKernelGGL((sdp_stream_dkv_kernel<NDT>), dim3((unsigned)(p.Bq * p.H), (unsigned)((p.Tk + 63) / 64)),
                       dim3(256), lds_kv, st, s);
}

static bool st_vec_ok(const void* ptr, int64_t bs) { return nm_aligned16(ptr) && (bs & 3) == 0; }

// the checks the two entry points share; 0 or the error code with the text set
static int st_check(const char* who, int64_t Bq, int64_t rpk, int64_t Tq, int64_t Tk, int64_t H, int64_t dh,
                    float keep_prob) {
    NM_REQUIRE(Bq > 0 && rpk >= 1 && Tq > 0 && Tk > 0 && H > 0 && dh > 0,
               "%s: bad shape Bq=%ld rows_per_key=%ld Tq=%ld Tk=%ld H=%ld dh=%ld", who, (long)Bq, (long)rpk, (long)Tq,
               (long)Tk, (long)H, (long)dh);
    NM_REQUIRE(Bq % rpk == 0, "%s: Bq=%ld is no multiple of rows_per_key=%ld", who, (long)Bq, (long)rpk);
    NM_REQUIRE(dh == 16 || dh == 32 || dh == 64 || dh == 128, "%s: dh=%ld must be 16, 32, 64 or 128", who, (long)dh);
    NM_REQUIRE(keep_prob > 0.0f && keep_prob <= 1.0f, "%s: keep_prob %g outside (0,1]", who, keep_prob);
    NM_REQUIRE(Bq * H < (1LL << 31) && Tq <= 65535LL * ST_TILE && Tk <= 65535LL * ST_TILE, "%s: grid too large", who);
    NM_REQUIRE(keep_prob >= 1.0f || (double)Bq * H * Tq * Tk < 4294967296.0, "%s: dropout mask index overflow", who);
    return NM_OK;
}

static void st_fill(SdpArgs& p, const float* q, int64_t q_bs, const float* k, int64_t k_bs, const float* v,
                    int64_t v_bs, const float* mask, int64_t mask_bs, int64_t Bq, int64_t rpk, int64_t Tq, int64_t Tk,
                    int64_t H, int64_t dh, int causal, float keep_prob, uint32_t salt, const uint32_t* step) {
    p.q = q; p.q_bs = q_bs; p.k = k; p.k_bs = k_bs; p.v = v; p.v_bs = v_bs;
    p.mask = mask; p.mask_bs = mask_bs; p.ctx = nullptr; p.ctx_bs = 0; p.weights = nullptr;
    p.Bq = (int)Bq; p.rpk = (int)rpk; p.Tq = (int)Tq; p.Tk = (int)Tk; p.H = (int)H; p.dh = (int)dh; p.causal = causal;
    p.scale = 1.0f / sqrtf((float)dh);
    p.keep_prob = keep_prob; p.inv_keep = 1.0f / keep_prob; p.salt = salt; p.step = step;
}

extern "C" int nm_sdp_stream_wanted(int64_t Tq, int64_t Tk, int64_t dh, int backward) {
    if (Tq <= 0 || Tk <= 0 || dh <= 0) return 0;
    if (sdp_fwd_lds(Tk, dh) > NM_SDP_LDS_LIMIT) return 1;
    return backward && sdp_bwd_lds(Tq, Tk, dh) > NM_SDP_LDS_LIMIT ? 1 : 0;
}

extern "C" int64_t nm_sdp_stream_workspace_bytes(int64_t Bq, int64_t H, int64_t Tq) {
    if (Bq <= 0 || H <= 0 || Tq <= 0) return 0;
    return (int64_t)sizeof(float) * Bq * H * Tq;
}

extern "C" int nm_sdp_stream_fwd(void* stream, const float* q, int64_t q_bs, const float* k, int64_t k_bs,
                                 const float* v, int64_t v_bs, const float* key_mask, int64_t mask_bs, int64_t Bq,
                                 int64_t rows_per_key, int64_t Tq, int64_t Tk, int64_t H, int64_t dh, int causal,
                                 float keep_prob, uint32_t salt, const uint32_t* step, float* ctx, int64_t ctx_bs,
                                 float* weights, float* row_max, float* row_sum) {
    const char* who = "nm_sdp_stream_fwd";
    NM_REQUIRE(q && k && v && ctx && !row_max == !row_sum, "%s: null pointer", who);
    if (int rc = st_check(who, Bq, rows_per_key, Tq, Tk, H, dh, keep_prob)) return rc;
    NM_REQUIRE(st_vec_ok(q, q_bs) && st_vec_ok(k, k_bs) && st_vec_ok(v, v_bs) && st_vec_ok(ctx, ctx_bs),
               "%s: q, k, v and ctx must start on 16 bytes and have batch strides that are multiples of 4 floats", who);
    SdpArgs p;
    st_fill(p, q, q_bs, k, k_bs, v, v_bs, key_mask, mask_bs, Bq, rows_per_key, Tq, Tk, H, dh, causal, keep_prob, salt,
            step);
    p.ctx = ctx; p.ctx_bs = ctx_bs; p.weights = weights;
    hipStream_t st = nm_stream(stream);
    // one query per row, no dropout, no backward to follow: the wave-per-(row, head) kernel streams the keys from
    // global memory with an online softmax of its own
    if (Tq == 1 && keep_prob >= 1.0f && !row_max && nm_cur()->sw.sdp_decode && nm_sdp_decode_launch(p, nullptr, 0, st)) {
        NM_LAUNCH_CHECK("nm_sdp_stream_fwd (decode)");
    }
    switch (dh) {
        case 16: st_launch_fwd<1>(p, row_max, row_sum, st); break;
        case 32: st_launch_fwd<2>(p, row_max, row_sum, st); break;
        case 64: st_launch_fwd<4>(p, row_max, row_sum, st); break;
        default: st_launch_fwd<8>(p, row_max, row_sum, st); break;
    }
    NM_LAUNCH_CHECK("nm_sdp_stream_fwd");
}

extern "C" int nm_sdp_stream_bwd(void* stream, const float* q, int64_t q_bs, const float* k, int64_t k_bs,
                                 const float* v, int64_t v_bs, const float* key_mask, int64_t mask_bs, const float* ctx,
                                 int64_t ctx_bs, const float* row_max, const float* row_sum, const float* dctx,
                                 int64_t dctx_bs, int64_t B, int64_t rows_per_key, int64_t Tq, int64_t Tk, int64_t H,
                                 int64_t dh, int causal, float keep_prob, uint32_t salt, const uint32_t* step,
                                 float* dq, int64_t dq_bs, float* dk, int64_t dk_bs, float* dv, int64_t dv_bs,
                                 float* workspace, int accumulate) {
    const char* who = "nm_sdp_stream_bwd";
    NM_REQUIRE(q && k && v && ctx && row_max && row_sum && dctx && dq && dk && dv && workspace, "%s: null pointer",
               who);
    if (int rc = st_check(who, B, rows_per_key, Tq, Tk, H, dh, keep_prob)) return rc;
    NM_REQUIRE(rows_per_key == 1, "%s: rows_per_key=%ld must be 1", who, (long)rows_per_key);
    NM_REQUIRE(st_vec_ok(q, q_bs) && st_vec_ok(k, k_bs) && st_vec_ok(v, v_bs) && st_vec_ok(ctx, ctx_bs) &&
                   st_vec_ok(dctx, dctx_bs) && st_vec_ok(dq, dq_bs) && st_vec_ok(dk, dk_bs) && st_vec_ok(dv, dv_bs),
               "%s: q, k, v, ctx, dctx, dq, dk and dv must start on 16 bytes and have batch strides that are multiples "
               "of 4 floats", who);
    SdpStreamBwdArgs s;
    st_fill(s.a.f, q, q_bs, k, k_bs, v, v_bs, key_mask, mask_bs, B, 1, Tq, Tk, H, dh, causal, keep_prob, salt, step);
    s.a.dctx = dctx; s.a.dctx_bs = dctx_bs; s.a.dq = dq; s.a.dq_bs = dq_bs; s.a.dk = dk; s.a.dk_bs = dk_bs;
    s.a.dv = dv; s.a.dv_bs = dv_bs; s.a.de = workspace; s.a.accumulate = accumulate;
    s.row_max = row_max; s.row_sum = row_sum;
    hipStream_t st = nm_stream(stream);
    const long total = B * H * Tq;
    const long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(sdp_stream_dsum_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, ctx,
                       (long)ctx_bs, dctx, (long)dctx_bs, workspace, (int)H, (int)dh, (int)Tq, total);
    switch (dh) {
        case 16: st_launch_bwd<1>(s, st); break;
        case 32: st_launch_bwd<2>(s, st); break;
        case 64: st_launch_bwd<4>(s, st); break;
        default: st_launch_bwd<8>(s, st); break;
    }
    NM_LAUNCH_CHECK("nm_sdp_stream_bwd");
}
