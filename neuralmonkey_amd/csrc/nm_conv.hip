// Sentence-CNN encoder front end on the gfx950 matrix cores (v_mfma_f32_32x32x2_f32: exact f32).  Replaces
//   encoders/sentence_cnn_encoder.py:103-143   (dropout -> per filter width tf.nn.conv1d SAME + bias_add + relu ->
//                                               tf.nn.max_pool SAME over segments -> concat)
//   encoders/sentence_cnn_encoder.py:188-196   (SAME max-pool of the token mask; ceil(len / s) of :164-167)
//   nn/highway.py:6-57                         (the point-wise part of a highway layer)
// and their tf.gradients.
//
// Layouts (row-major fp32): x [B, S, E]; filter i: W_i [w_i, E, n_i] (TF's conv1d filter), b_i [n_i];
// pooled / argmax [B, S', ldp] with width i in columns [col_i, col_i + n_i); S' = ceil(S / s); SAME pooling pads
// (S' s - S) / 2 positions before the first window, so window j covers t in [j s - pb, j s - pb + s) n [0, S).
// SAME convolution pads (w - 1) / 2 positions before and the rest after.
//
// Kernels
//   conv_mfma<false>  forward: one launch for every filter width.  A workgroup owns 128 positions of one sentence
//                     (whole pooling windows) x 64 filters of one width; per chunk of 16 input channels it stages
//                     the positions plus the w - 1 halo rows once in LDS and reads them shifted for every tap
//                     (implicit GEMM, K = w E, no im2col).  Epilogue: bias, relu, segment max + argmax (ties to the
//                     lowest t, TF's order) straight into the pooled output.
//   conv_mfma<true>   data gradient: the transposed convolution of all widths accumulated in one tile of dx;
//                     the workgroup loops over widths x chunks of 16 filters.
//   conv_wgrad_mfma   weight gradient per (width, tap, 64 channels, 64 filters) tile, positions split over
//                     workgroups into fixed slabs that conv_wgrad_reduce sums in a fixed order: no float atomics,
//                     repeated runs are bit-identical.
//   *_generic         scalar kernels for shapes the MFMA path does not take (w > 8, s > 128).  No kernel takes more
//                     than 16 filter widths (CONV_MAX_WIDTHS, the table in ConvArgs): conv_setup refuses them.
//   convs2s_*         the residual layer of the convolutional sequence-to-sequence encoder (facebook_conv.py): the same
//                     implicit GEMM with a GLU + residual epilogue in registers; its gradients reuse conv_mfma<true>
//                     and the weight-gradient kernels through conv_grads_launch (further down).
#include "nm_common.h"
#include "../../include/nmhip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define CONV_MAX_WIDTHS 16
#define CONV_FAST_MAX_W 8
#define CONV_BM 128          // positions per workgroup tile (4 waves x 32)
#define CONV_BN 64           // output columns per workgroup tile (2 MFMA tiles per wave)
#define CONV_CH 16           // input channels per LDS stage
#define CONV_XR (CONV_BM + CONV_FAST_MAX_W - 1 + 1)   // staged rows (tile + halo), padded
#define WG_BM 64             // weight gradient: channels per tile
#define WG_BN 64             // weight gradient: filters per tile
#define WG_PC 32             // weight gradient: positions per LDS stage

struct ConvWidth {
    const float* W;          // [w, E, n]
    const float* bias;       // [n] (forward) or null
    float* dW;               // weight gradient [w, E, n] (backward)
    int w, n, col;           // width, filters, first column in the pooled output
    int tile0;               // first workgroup tile of this width (grid.y of the forward, grid.x of the weight gradient)
};

struct ConvArgs {
    const float* x;          // [B, S, E] rows of ldx floats (forward input / weight-gradient input)
    long ldx;
    const float* dz;         // [B, S, ldp] dense pre-activation gradient (backward)
    float* dx;               // [B, S, E] rows of lddx floats (data gradient)
    long lddx;
    int B, S, E, s, Sp, pb;
    int ldp;                 // columns of pooled / argmax / dz (sum of the filter counts)
    int nw;
    ConvWidth wd[CONV_MAX_WIDTHS];
    float* pooled;
    int* argmax;
    int accumulate;          // data gradient: dx += ...
    float* ws;               // weight gradient slabs [slices][sum_i w_i E n_i]
    long ws_slab;            // floats per slab
    int slices;
    int tiles_total;         // weight gradient tiles (grid.x)
};

__device__ __forceinline__ int conv_width_of_tile(const ConvArgs& a, int tile) {
    int i = 0;
    while (i + 1 < a.nw && a.wd[i + 1].tile0 <= tile) ++i;
    return i;
}

// ---------------------------------------------------------------------------------------------------------------
// forward (BWD = false) and data gradient (BWD = true) as one implicit-GEMM anatomy
// ---------------------------------------------------------------------------------------------------------------
template <bool BWD>
__global__ __launch_bounds__(256) void conv_mfma(ConvArgs a) {
    constexpr int OP_FLOATS = CONV_CH * CONV_XR + CONV_FAST_MAX_W * CONV_CH * CONV_BN;
    constexpr int EP_FLOATS = BWD ? 0 : CONV_BM * (CONV_BN + 1);
    constexpr int SM_FLOATS = OP_FLOATS > EP_FLOATS ? OP_FLOATS : EP_FLOATS;
    __shared__ __attribute__((aligned(16))) float smem[SM_FLOATS];
    float (*Xs)[CONV_XR] = reinterpret_cast<float (*)[CONV_XR]>(smem);                       // [ch][row]
    float (*Ws)[CONV_CH][CONV_BN] = reinterpret_cast<float (*)[CONV_CH][CONV_BN]>(smem + CONV_CH * CONV_XR);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // tiles of positions: forward in whole pooling windows (P windows of s positions), backward plain 128 rows
    const int P = BWD ? 0 : CONV_BM / a.s;
    const int tiles_t = BWD ? (a.S + CONV_BM - 1) / CONV_BM : (a.Sp + P - 1) / P;
    const int b = blockIdx.x / tiles_t, tt = blockIdx.x % tiles_t;
    const int j0 = BWD ? 0 : tt * P;
    const int t0 = BWD ? tt * CONV_BM : j0 * a.s - a.pb;
    int wi0, wi1, n0, ncols;
    if (BWD) {
        wi0 = 0; wi1 = a.nw; n0 = blockIdx.y * CONV_BN; ncols = a.E;
    } else {
        wi0 = conv_width_of_tile(a, blockIdx.y); wi1 = wi0 + 1;
        n0 = (blockIdx.y - a.wd[wi0].tile0) * CONV_BN; ncols = a.wd[wi0].n;
    }

    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;

    for (int wi = wi0; wi < wi1; ++wi) {
        const ConvWidth cw = a.wd[wi];
        const int w = cw.w, pad = (w - 1) / 2;
        // first staged row: forward t0 - pad (tap k reads row r + k); backward t0 - (w - 1 - pad) (tap k: r + w-1-k)
        const int tstage = BWD ? t0 - (w - 1 - pad) : t0 - pad;
        const int nrows = CONV_BM + w - 1;
        const int cin = BWD ? cw.n : a.E;                    // channels of the staged operand
        for (int c0 = 0; c0 < cin; c0 += CONV_CH) {
            // stage the input rows: channel fastest (contiguous in global memory)
            for (int idx = tid; idx < CONV_CH * nrows; idx += 256) {
                const int c = idx % CONV_CH, r = idx / CONV_CH;
                const int t = tstage + r;
                float v = 0.0f;
                if (t >= 0 && t < a.S && c0 + c < cin) {
                    const long row = (long)b * a.S + t;
                    v = BWD ? a.dz[row * a.ldp + cw.col + c0 + c] : a.x[row * a.ldx + c0 + c];
                }
                Xs[c][r] = v;
            }
            // stage the filter taps: Ws[k][c][o] = W[k][c0 + c][n0 + o] (forward) / W[k][n0 + o][c0 + c] (backward)
            for (int idx = tid; idx < w * CONV_CH * CONV_BN; idx += 256) {
                int k, c, o;
                if (BWD) { c = idx % CONV_CH; o = (idx / CONV_CH) % CONV_BN; k = idx / (CONV_CH * CONV_BN); }
                else     { o = idx % CONV_BN; c = (idx / CONV_BN) % CONV_CH; k = idx / (CONV_CH * CONV_BN); }
                float v = 0.0f;
                if (c0 + c < cin && n0 + o < ncols)
                    v = BWD ? cw.W[((long)k * a.E + n0 + o) * cw.n + c0 + c]
                            : cw.W[((long)k * a.E + c0 + c) * cw.n + n0 + o];
                Ws[k][c][o] = v;
            }
            __syncthreads();
            const int m = wave * 32 + (lane & 31), kr = lane >> 5;
            for (int k = 0; k < w; ++k) {
                const int shift = BWD ? w - 1 - k : k;
#pragma unroll
                for (int cc = 0; cc < CONV_CH; cc += 2) {
                    const float av = Xs[cc + kr][m + shift];
                    const float b0 = Ws[k][cc + kr][lane & 31];
                    const float b1 = Ws[k][cc + kr][32 + (lane & 31)];
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc[1], 0, 0, 0);
                }
            }
            __syncthreads();
        }
    }

    // C/D layout of v_mfma_f32_32x32x2_f32: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    if (BWD) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int e = n0 + j * 32 + (lane & 31);
            if (e >= a.E) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int t = t0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (t < a.S) {
                    float* p = a.dx + ((long)b * a.S + t) * a.lddx + e;
                    *p = a.accumulate ? *p + acc[j][r] : acc[j][r];
                }
            }
        }
        return;
    }
    const ConvWidth cw = a.wd[wi0];
    float (*Cs)[CONV_BN + 1] = reinterpret_cast<float (*)[CONV_BN + 1]>(smem);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int o = j * 32 + (lane & 31);
        const float bv = (n0 + o < cw.n && cw.bias) ? cw.bias[n0 + o] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            Cs[row][o] = fmaxf(acc[j][r] + bv, 0.0f);
        }
    }
    __syncthreads();
    for (int idx = tid; idx < P * CONV_BN; idx += 256) {
        const int p = idx / CONV_BN, o = idx % CONV_BN;
        const int jw = j0 + p;
        if (jw >= a.Sp || n0 + o >= cw.n) continue;
        float best = -1.0f;
        int arg = 0;
        for (int i = 0; i < a.s; ++i) {
            const int t = t0 + p * a.s + i;
            if (t < 0 || t >= a.S) continue;
            const float v = Cs[p * a.s + i][o];
            if (v > best) { best = v; arg = t; }
        }
        const long out = ((long)b * a.Sp + jw) * a.ldp + cw.col + n0 + o;
        a.pooled[out] = best;
        a.argmax[out] = arg;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// scalar forward / data gradient: any width, any segment size
// ---------------------------------------------------------------------------------------------------------------
__global__ void conv_fwd_generic(ConvArgs a) {
    const long total = (long)a.B * a.Sp * a.ldp;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int col = (int)(i % a.ldp);
        const long bj = i / a.ldp;
        const int jw = (int)(bj % a.Sp), b = (int)(bj / a.Sp);
        int wi = 0;
        while (wi + 1 < a.nw && a.wd[wi + 1].col <= col) ++wi;
        const ConvWidth cw = a.wd[wi];
        const int o = col - cw.col, pad = (cw.w - 1) / 2;
        float best = -1.0f;
        int arg = 0;
        for (int q = 0; q < a.s; ++q) {
            const int t = jw * a.s - a.pb + q;
            if (t < 0 || t >= a.S) continue;
            float v = 0.0f;
            for (int k = 0; k < cw.w; ++k) {
                const int tk = t + k - pad;
                if (tk < 0 || tk >= a.S) continue;
                const float* xr = a.x + ((long)b * a.S + tk) * a.ldx;
                const float* wr = cw.W + (long)k * a.E * cw.n + o;
                for (int e = 0; e < a.E; ++e) v = fmaf(xr[e], wr[(long)e * cw.n], v);
            }
            v = fmaxf(v + (cw.bias ? cw.bias[o] : 0.0f), 0.0f);
            if (v > best) { best = v; arg = t; }
        }
        a.pooled[i] = best;
        a.argmax[i] = arg;
    }
}

__global__ void conv_bwd_data_generic(ConvArgs a) {
    const long total = (long)a.B * a.S * a.E;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int e = (int)(i % a.E);
        const long bt = i / a.E;
        const int t = (int)(bt % a.S), b = (int)(bt / a.S);
        float v = 0.0f;
        for (int wi = 0; wi < a.nw; ++wi) {
            const ConvWidth cw = a.wd[wi];
            const int pad = (cw.w - 1) / 2;
            for (int k = 0; k < cw.w; ++k) {
                const int to = t - k + pad;             // the output position that read x[t] through tap k
                if (to < 0 || to >= a.S) continue;
                const float* zr = a.dz + ((long)b * a.S + to) * a.ldp + cw.col;
                const float* wr = cw.W + ((long)k * a.E + e) * cw.n;
                for (int f = 0; f < cw.n; ++f) v = fmaf(zr[f], wr[f], v);
            }
        }
        float* p = a.dx + bt * a.lddx + e;
        *p = a.accumulate ? *p + v : v;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// weight gradient: dW_i[k, e, f] = sum_{b, t} x[b, t + k - pad_i, e] dz[b, t, col_i + f]
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void conv_wgrad_mfma(ConvArgs a) {
    __shared__ __attribute__((aligned(16))) float Xs[WG_PC][WG_BM + 4];
    __shared__ __attribute__((aligned(16))) float Zs[WG_PC][WG_BN + 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x;
    const int wi = conv_width_of_tile(a, tile);
    const ConvWidth cw = a.wd[wi];
    const int te = (a.E + WG_BM - 1) / WG_BM, tf = (cw.n + WG_BN - 1) / WG_BN;
    int rem = tile - cw.tile0;
    const int k = rem / (te * tf);
    rem %= te * tf;
    const int e0 = (rem / tf) * WG_BM, f0 = (rem % tf) * WG_BN;
    const int pad = (cw.w - 1) / 2;
    const long npos = (long)a.B * a.S;
    const long per = (npos + a.slices - 1) / a.slices;
    const long p0 = blockIdx.y * per, p1 = p0 + per < npos ? p0 + per : npos;

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    for (long pc = p0; pc < p1; pc += WG_PC) {
        for (int idx = tid; idx < WG_PC * WG_BM; idx += 256) {
            const int pp = idx / WG_BM, e = idx % WG_BM;
            const long p = pc + pp;
            float v = 0.0f;
            if (p < p1 && e0 + e < a.E) {
                const int b = (int)(p / a.S), t = (int)(p % a.S) + k - pad;
                if (t >= 0 && t < a.S) v = a.x[((long)b * a.S + t) * a.ldx + e0 + e];
            }
            Xs[pp][e] = v;
        }
        for (int idx = tid; idx < WG_PC * WG_BN; idx += 256) {
            const int pp = idx / WG_BN, f = idx % WG_BN;
            const long p = pc + pp;
            Zs[pp][f] = (p < p1 && f0 + f < cw.n) ? a.dz[p * a.ldp + cw.col + f0 + f] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < WG_PC; kk += 2) {
            const float av = Xs[kk + (lane >> 5)][wm + (lane & 31)];
            const float bv = Zs[kk + (lane >> 5)][wn + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    // slab of this slice; layout of width i: [w_i, E, n_i] at the width's offset (tile-independent)
    long off = 0;
    for (int i = 0; i < wi; ++i) off += (long)a.wd[i].w * a.E * a.wd[i].n;
    float* slab = a.ws + blockIdx.y * a.ws_slab + off + (long)k * a.E * cw.n;
    const int f = f0 + wn + (lane & 31);
    if (f >= cw.n) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int e = e0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (e < a.E) slab[(long)e * cw.n + f] = acc[r];
    }
}

__global__ void conv_wgrad_generic(ConvArgs a) {
    // one thread per weight: the slab of slice 0 receives the whole sum
    const long total = a.ws_slab;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        long r = i;
        int wi = 0;
        while (r >= (long)a.wd[wi].w * a.E * a.wd[wi].n) { r -= (long)a.wd[wi].w * a.E * a.wd[wi].n; ++wi; }
        const ConvWidth cw = a.wd[wi];
        const int f = (int)(r % cw.n), e = (int)((r / cw.n) % a.E), k = (int)(r / ((long)cw.n * a.E));
        const int pad = (cw.w - 1) / 2;
        float v = 0.0f;
        for (int b = 0; b < a.B; ++b)
            for (int t = 0; t < a.S; ++t) {
                const int tk = t + k - pad;
                if (tk < 0 || tk >= a.S) continue;
                v = fmaf(a.x[((long)b * a.S + tk) * a.ldx + e], a.dz[((long)b * a.S + t) * a.ldp + cw.col + f], v);
            }
        a.ws[i] = v;
    }
}

// dW_i (+)= sum over slabs in slab order
__global__ void conv_wgrad_reduce(ConvArgs a, int accumulate) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < a.ws_slab; i += (long)gridDim.x * blockDim.x) {
        float v = 0.0f;
        for (int z = 0; z < a.slices; ++z) v += a.ws[z * a.ws_slab + i];
        long r = i;
        int wi = 0;
        while (r >= (long)a.wd[wi].w * a.E * a.wd[wi].n) { r -= (long)a.wd[wi].w * a.E * a.wd[wi].n; ++wi; }
        float* p = a.wd[wi].dW + r;
        *p = accumulate ? *p + v : v;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// point-wise parts of the backward pass and the pooled mask
// ---------------------------------------------------------------------------------------------------------------
// dz[b, t, c] for every position of window j: dpooled routed to the argmax, gated by pooled > 0 (TF's ReluGrad on the
// relu output); every element of dz is written exactly once, so no clearing launch is needed.  The bias gradient is
// the column sum of the gated pooled gradient (conv_bias_grad).
__global__ void conv_route_grad(const float* __restrict__ dpooled, const float* __restrict__ pooled,
                                const int* __restrict__ argmax, float* __restrict__ dz, int B, int S, int Sp, int s,
                                int pb, int ldp) {
    const long total = (long)B * Sp * ldp;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % ldp);
        const long bj = i / ldp;
        const int jw = (int)(bj % Sp), b = (int)(bj / Sp);
        const float g = pooled[i] > 0.0f ? dpooled[i] : 0.0f;
        const int arg = argmax[i];
        for (int q = 0; q < s; ++q) {
            const int t = jw * s - pb + q;
            if (t < 0 || t >= S) continue;
            dz[((long)b * S + t) * ldp + c] = t == arg ? g : 0.0f;
        }
    }
}

// a workgroup owns 16 columns; its 16 row lanes sum every 16th row, the lanes are added in a fixed order
#define BG_COLS 16
#define BG_LANES 16
__global__ __launch_bounds__(BG_COLS * BG_LANES) void conv_bias_grad(const float* __restrict__ dpooled,
                                                                    const float* __restrict__ pooled, int rows,
                                                                    int ldp, ConvArgs a, int accumulate) {
    __shared__ float part[BG_LANES][BG_COLS];
    const int cl = threadIdx.x % BG_COLS, lane = threadIdx.x / BG_COLS;
    const int c = blockIdx.x * BG_COLS + cl;
    float v = 0.0f;
    if (c < ldp)
        for (int r = lane; r < rows; r += BG_LANES) {
            const long i = (long)r * ldp + c;
            if (pooled[i] > 0.0f) v += dpooled[i];
        }
    part[lane][cl] = v;
    __syncthreads();
    if (lane != 0 || c >= ldp) return;
    v = 0.0f;
    for (int l = 0; l < BG_LANES; ++l) v += part[l][cl];
    int wi = 0;
    while (wi + 1 < a.nw && a.wd[wi + 1].col <= c) ++wi;
    float* p = const_cast<float*>(a.wd[wi].bias) + (c - a.wd[wi].col);
    *p = accumulate ? *p + v : v;
}

// mask_out[b, j] = max over window j of mask[b, t]; seq_lens[b] = ceil(lengths[b] / s)
__global__ void conv_pool_mask(const float* __restrict__ mask, const int* __restrict__ lengths, float* mask_out,
                               int* seq_lens, int B, int S, int Sp, int s, int pb) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (long)B * Sp && mask_out) {
        const int jw = (int)(i % Sp), b = (int)(i / Sp);
        float best = -INFINITY;
        for (int q = 0; q < s; ++q) {
            const int t = jw * s - pb + q;
            if (t >= 0 && t < S) best = fmaxf(best, mask[(long)b * S + t]);
        }
        mask_out[i] = best;
    }
    if (i < B && seq_lens) seq_lens[i] = (lengths[i] + s - 1) / s;
}

// highway (nn/highway.py:44-57): T = sigmoid(zt + bt), H = relu(zh + bh), y = H T + x (1 - T); T and H kept
__global__ void highway_fwd_kernel(const float* __restrict__ zt, const float* __restrict__ zh,
                                   const float* __restrict__ x, const float* __restrict__ bt,
                                   const float* __restrict__ bh, float* __restrict__ y, float* __restrict__ tsave,
                                   float* __restrict__ hsave, long rows, int cols, long ldz, long ldx) {
    const long total = rows * cols;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / cols;
        const int c = (int)(i - r * cols);
        const float t = 1.0f / (1.0f + expf(-(zt[r * ldz + c] + bt[c])));
        const float h = fmaxf(zh[r * ldz + c] + bh[c], 0.0f);
        const float xv = x[r * ldx + c];
        y[r * ldx + c] = h * t + xv * (1.0f - t);
        tsave[i] = t;
        hsave[i] = h;
    }
}

// dzt = dy (H - x) T (1 - T); dzh = dy T [H > 0]; dx (+)= dy (1 - T)
__global__ void highway_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                   const float* __restrict__ tsave, const float* __restrict__ hsave,
                                   float* __restrict__ dzt, float* __restrict__ dzh, float* __restrict__ dx,
                                   long rows, int cols, long ldx, long ldz, int accumulate) {
    const long total = rows * cols;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / cols;
        const int c = (int)(i - r * cols);
        const float g = dy[r * ldx + c], t = tsave[i], h = hsave[i], xv = x[r * ldx + c];
        dzt[r * ldz + c] = g * (h - xv) * t * (1.0f - t);
        dzh[r * ldz + c] = h > 0.0f ? g * t : 0.0f;
        const float d = g * (1.0f - t);
        dx[r * ldx + c] = accumulate ? dx[r * ldx + c] + d : d;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
static int ew_grid(long n) {
    long g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

static int conv_setup(const char* what, ConvArgs& a, int B, int S, int E, int s, int nw, const int* widths,
                      const int* counts, const float* const* W, int64_t ldp) {
    NM_REQUIRE(B > 0 && S > 0 && E > 0 && s > 0, "%s: bad sizes B=%d S=%d E=%d s=%d", what, B, S, E, s);
    NM_REQUIRE(nw >= 1 && nw <= CONV_MAX_WIDTHS, "%s: %d filter widths (1..%d)", what, nw, CONV_MAX_WIDTHS);
    NM_REQUIRE(widths && counts && W, "%s: null filter table", what);
    memset(&a, 0, sizeof(a));
    a.B = B; a.S = S; a.E = E; a.s = s;
    a.Sp = (S + s - 1) / s;
    a.pb = (a.Sp * s - S) / 2;
    a.nw = nw;
    int col = 0;
    for (int i = 0; i < nw; ++i) {
        NM_REQUIRE(widths[i] > 0 && counts[i] > 0, "%s: filter %d has width %d, count %d", what, i, widths[i], counts[i]);
        NM_REQUIRE(W[i], "%s: null filter %d", what, i);
        a.wd[i].W = W[i];
        a.wd[i].w = widths[i];
        a.wd[i].n = counts[i];
        a.wd[i].col = col;
        col += counts[i];
    }
    NM_REQUIRE(ldp == col, "%s: pooled width %lld != sum of filter counts %d", what, (long long)ldp, col);
    a.ldp = col;
    return NM_OK;
}

static bool conv_fast_ok(const ConvArgs& a) {
    if (a.s > CONV_BM) return false;
    for (int i = 0; i < a.nw; ++i)
        if (a.wd[i].w > CONV_FAST_MAX_W) return false;
    return true;
}

extern "C" int nm_conv1d_pool_fwd(void* stream, const float* x, int64_t ldx, int B, int S, int E, int segment,
                                  int nw, const int* widths, const int* counts, const float* const* W,
                                  const float* const* bias, float* pooled, int* argmax, int64_t ldp,
                                  const float* mask, const int* lengths, float* mask_out, int* seq_lens, int algo) {
    ConvArgs a;
    int rc = conv_setup("nm_conv1d_pool_fwd", a, B, S, E, segment, nw, widths, counts, W, ldp);
    if (rc) return rc;
    NM_REQUIRE(x && pooled && argmax && bias, "nm_conv1d_pool_fwd: null operand");
    NM_REQUIRE(ldx >= E, "nm_conv1d_pool_fwd: ldx %lld < E %d", (long long)ldx, E);
    NM_REQUIRE(!mask_out || mask, "nm_conv1d_pool_fwd: mask_out needs the mask");
    NM_REQUIRE(!seq_lens || lengths, "nm_conv1d_pool_fwd: seq_lens needs the lengths");
    NM_REQUIRE(algo >= 0 && algo <= 2, "nm_conv1d_pool_fwd: algo %d (0 auto, 1 mfma, 2 generic)", algo);
    for (int i = 0; i < nw; ++i) NM_REQUIRE(bias[i], "nm_conv1d_pool_fwd: null bias %d", i);
    a.x = x; a.ldx = ldx; a.pooled = pooled; a.argmax = argmax;
    const bool fast = conv_fast_ok(a);
    NM_REQUIRE(algo != 1 || fast, "nm_conv1d_pool_fwd: the MFMA kernel takes widths <= %d and segments <= %d",
               CONV_FAST_MAX_W, CONV_BM);
    hipStream_t st = nm_stream(stream);
    if (fast && algo != 2) {
        int tiles = 0;
        for (int i = 0; i < nw; ++i) {
            a.wd[i].bias = bias[i];
            a.wd[i].tile0 = tiles;
            tiles += (a.wd[i].n + CONV_BN - 1) / CONV_BN;
        }
        const int P = CONV_BM / segment;
        const long gx = (long)B * ((a.Sp + P - 1) / P);
        NM_REQUIRE(gx < (1L << 31), "nm_conv1d_pool_fwd: grid too large");
        hipLaunchKernelGGL(conv_mfma<false>, dim3((unsigned)gx, tiles), dim3(256), 0, st, a);
    } else {
        for (int i = 0; i < nw; ++i) a.wd[i].bias = bias[i];
        hipLaunchKernelGGL(conv_fwd_generic, dim3(ew_grid((long)B * a.Sp * a.ldp)), dim3(256), 0, st, a);
    }
    if (mask_out || seq_lens) {
        const long n = (long)B * a.Sp > B ? (long)B * a.Sp : B;
        hipLaunchKernelGGL(conv_pool_mask, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, mask, lengths,
                           mask_out, seq_lens, B, S, a.Sp, segment, a.pb);
    }
    NM_LAUNCH_CHECK("nm_conv1d_pool_fwd");
}

extern "C" int64_t nm_conv1d_wgrad_workspace_bytes(int B, int S, int E, int nw, const int* widths, const int* counts) {
    if (B <= 0 || S <= 0 || E <= 0 || nw <= 0 || nw > CONV_MAX_WIDTHS || !widths || !counts) return 0;
    long slab = 0, tiles = 0;
    for (int i = 0; i < nw; ++i) {
        slab += (long)widths[i] * E * counts[i];
        tiles += (long)widths[i] * ((E + WG_BM - 1) / WG_BM) * ((counts[i] + WG_BN - 1) / WG_BN);
    }
    // slices: about 2048 workgroups, at least 256 positions each, at most 32 slabs
    long npos = (long)B * S;
    long slices = (2048 + tiles - 1) / tiles;
    if (slices > npos / 256) slices = npos / 256;
    if (slices > 32) slices = 32;
    if (slices < 1) slices = 1;
    return slices * slab * (int64_t)sizeof(float);
}

// The data gradient and the weight gradient of a prepared ConvArgs whose dz is written (x, ldx, dz, dx, lddx, accumulate
// set): dx (+)= the transposed convolution of every width when a.dx is given; dW_i (+)= the fixed-order slab sums when
// dW is given (``need`` = nm_conv1d_wgrad_workspace_bytes of the shape).  Shared by nm_conv1d_pool_bwd and
// nm_conv1d_glu_bwd.
static void conv_grads_launch(hipStream_t st, ConvArgs& a, bool mfma, float* const* dW, int64_t need, void* workspace,
                              int accumulate_params) {
    if (a.dx) {
        if (mfma)
            hipLaunchKernelGGL(conv_mfma<true>,
                               dim3(a.B * ((a.S + CONV_BM - 1) / CONV_BM), (a.E + CONV_BN - 1) / CONV_BN), dim3(256), 0,
                               st, a);
        else
            hipLaunchKernelGGL(conv_bwd_data_generic, dim3(ew_grid((long)a.B * a.S * a.E)), dim3(256), 0, st, a);
    }
    if (!dW) return;
    long slab = 0;
    int tiles = 0;
    for (int i = 0; i < a.nw; ++i) {
        a.wd[i].dW = dW[i];
        a.wd[i].tile0 = tiles;
        tiles += a.wd[i].w * ((a.E + WG_BM - 1) / WG_BM) * ((a.wd[i].n + WG_BN - 1) / WG_BN);
        slab += (long)a.wd[i].w * a.E * a.wd[i].n;
    }
    a.ws = static_cast<float*>(workspace);
    a.ws_slab = slab;
    a.slices = mfma ? (int)(need / (int64_t)sizeof(float) / slab) : 1;
    a.tiles_total = tiles;
    if (mfma)
        hipLaunchKernelGGL(conv_wgrad_mfma, dim3(tiles, a.slices), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(conv_wgrad_generic, dim3(ew_grid(slab)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(conv_wgrad_reduce, dim3(ew_grid(slab)), dim3(256), 0, st, a, accumulate_params);
}

extern "C" int nm_conv1d_pool_bwd(void* stream, const float* x, int64_t ldx, int B, int S, int E, int segment,
                                  int nw, const int* widths, const int* counts, const float* const* W,
                                  const float* pooled, const int* argmax, const float* dpooled, int64_t ldp,
                                  float* dz, float* dx, int accumulate_dx, float* const* dW, float* const* dbias,
                                  int accumulate_params, void* workspace, int64_t workspace_bytes, int algo) {
    ConvArgs a;
    int rc = conv_setup("nm_conv1d_pool_bwd", a, B, S, E, segment, nw, widths, counts, W, ldp);
    if (rc) return rc;
    NM_REQUIRE(x && pooled && argmax && dpooled && dz, "nm_conv1d_pool_bwd: null operand");
    NM_REQUIRE(ldx >= E, "nm_conv1d_pool_bwd: ldx %lld < E %d", (long long)ldx, E);
    NM_REQUIRE(algo >= 0 && algo <= 2, "nm_conv1d_pool_bwd: algo %d (0 auto, 1 mfma, 2 generic)", algo);
    const bool params = dW != nullptr;
    if (params) {
        NM_REQUIRE(dbias && workspace, "nm_conv1d_pool_bwd: weight gradients need the bias gradients and a workspace");
        for (int i = 0; i < nw; ++i) NM_REQUIRE(dW[i] && dbias[i], "nm_conv1d_pool_bwd: null gradient %d", i);
    }
    const int64_t need = nm_conv1d_wgrad_workspace_bytes(B, S, E, nw, widths, counts);
    NM_REQUIRE(!params || workspace_bytes >= need, "nm_conv1d_pool_bwd: workspace too small (%lld < %lld bytes)",
               (long long)workspace_bytes, (long long)need);
    const bool fast = conv_fast_ok(a);
    NM_REQUIRE(algo != 1 || fast, "nm_conv1d_pool_bwd: the MFMA kernels take widths <= %d and segments <= %d",
               CONV_FAST_MAX_W, CONV_BM);
    const bool mfma = fast && algo != 2;
    a.x = x; a.ldx = ldx; a.dz = dz; a.dx = dx; a.lddx = ldx; a.accumulate = accumulate_dx;
    hipStream_t st = nm_stream(stream);
    hipLaunchKernelGGL(conv_route_grad, dim3(ew_grid((long)B * a.Sp * a.ldp)), dim3(256), 0, st, dpooled, pooled,
                       argmax, dz, B, S, a.Sp, segment, a.pb, a.ldp);
    for (int i = 0; params && i < nw; ++i) a.wd[i].bias = dbias[i];
    conv_grads_launch(st, a, mfma, params ? dW : nullptr, need, workspace, accumulate_params);
    if (params)
        hipLaunchKernelGGL(conv_bias_grad, dim3((a.ldp + BG_COLS - 1) / BG_COLS), dim3(BG_COLS * BG_LANES), 0, st,
                           dpooled, pooled, B * a.Sp, a.ldp, a, accumulate_params);
    NM_LAUNCH_CHECK("nm_conv1d_pool_bwd");
}

extern "C" int nm_highway_fwd(void* stream, const float* zt, const float* zh, int64_t ldz, const float* x,
                              int64_t ldx, const float* bt, const float* bh, float* y, float* tsave, float* hsave,
                              int64_t rows, int64_t cols) {
    NM_REQUIRE(zt && zh && x && bt && bh && y && tsave && hsave, "nm_highway_fwd: null operand");
    NM_REQUIRE(rows >= 0 && cols > 0 && ldz >= cols && ldx >= cols, "nm_highway_fwd: bad shape");
    NM_REQUIRE(y != x, "nm_highway_fwd: y may not overwrite x (the backward pass reads x)");
    if (rows == 0) return NM_OK;
    hipLaunchKernelGGL(highway_fwd_kernel, dim3(ew_grid(rows * cols)), dim3(256), 0, nm_stream(stream), zt, zh, x,
                       bt, bh, y, tsave, hsave, (long)rows, (int)cols, (long)ldz, (long)ldx);
    NM_LAUNCH_CHECK("nm_highway_fwd");
}

extern "C" int nm_highway_bwd(void* stream, const float* dy, const float* x, int64_t ldx, const float* tsave,
                              const float* hsave, float* dzt, float* dzh, int64_t ldz, float* dx, int64_t rows,
                              int64_t cols, int accumulate_dx) {
    NM_REQUIRE(dy && x && tsave && hsave && dzt && dzh && dx, "nm_highway_bwd: null operand");
    NM_REQUIRE(rows >= 0 && cols > 0 && ldz >= cols && ldx >= cols, "nm_highway_bwd: bad shape");
    if (rows == 0) return NM_OK;
    hipLaunchKernelGGL(highway_bwd_kernel, dim3(ew_grid(rows * cols)), dim3(256), 0, nm_stream(stream), dy, x, tsave,
                       hsave, dzt, dzh, dx, (long)rows, (int)cols, (long)ldx, (long)ldz, accumulate_dx);
    NM_LAUNCH_CHECK("nm_highway_bwd");
}

// ---------------------------------------------------------------------------------------------------------------
// ConvS2S residual layer (include/nmhip_convs2s.h): y = glu(conv1d_SAME(x, W) + bias) + x
//   encoders/facebook_conv.py:102-121, nn/projection.py:60-75
// x, y [B, T, C]; W [w, C, 2C]; bias [2C]: output feature c pairs the linear column c with the gate column C + c.
// ---------------------------------------------------------------------------------------------------------------
#define GLU_BC 32            // output features per workgroup tile; their gate partners fill the other 32 staged columns

struct GluArgs {
    const float* x;          // [B, T, C] rows of ldx floats
    long ldx;
    const float* W;          // [w, C, 2C]
    const float* bias;       // [2C]
    float* y;                // [B, T, C] rows of ldy floats
    long ldy;
    float* lin_save;         // [B T, C] contiguous or null
    float* sig_save;
    int B, T, C, w;
};

// one value of the layer from its two pre-activations (bias not yet added); the same expression in both kernels
__device__ __forceinline__ void glu_store(const GluArgs& a, long row, int c, float lin, float gate) {
    lin += a.bias[c];
    const float sig = 1.0f / (1.0f + expf(-(gate + a.bias[a.C + c])));
    a.y[row * a.ldy + c] = lin * sig + a.x[row * a.ldx + c];
    if (a.lin_save) {
        a.lin_save[row * a.C + c] = lin;
        a.sig_save[row * a.C + c] = sig;
    }
}

// Implicit GEMM as conv_mfma<false>: a workgroup owns 128 positions of one sentence x 32 output features; it stages the
// positions plus the w - 1 halo rows once per chunk of 16 input channels and reads them shifted for every tap.  The 64
// staged filter columns are the 32 linear columns and their 32 gate partners, so a wave's two accumulators hold the
// linear and the gate pre-activation of the same (t, c): bias, sigmoid, product, residual add and the optional saves
// happen in registers, and no [B, T, 2C] pre-activation reaches memory.
__global__ __launch_bounds__(256) void convs2s_glu_mfma(GluArgs a) {
    __shared__ __attribute__((aligned(16))) float smem[CONV_CH * CONV_XR + CONV_FAST_MAX_W * CONV_CH * CONV_BN];
    float (*Xs)[CONV_XR] = reinterpret_cast<float (*)[CONV_XR]>(smem);                       // [ch][row]
    float (*Ws)[CONV_CH][CONV_BN] = reinterpret_cast<float (*)[CONV_CH][CONV_BN]>(smem + CONV_CH * CONV_XR);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles_t = (a.T + CONV_BM - 1) / CONV_BM;
    const int b = blockIdx.x / tiles_t, t0 = (blockIdx.x % tiles_t) * CONV_BM;
    const int c0 = blockIdx.y * GLU_BC;
    const int w = a.w, pad = (w - 1) / 2, C = a.C;
    const int tstage = t0 - pad, nrows = CONV_BM + w - 1;
    const long n2 = 2L * C;

    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;

    for (int e0 = 0; e0 < C; e0 += CONV_CH) {
        for (int idx = tid; idx < CONV_CH * nrows; idx += 256) {
            const int e = idx % CONV_CH, r = idx / CONV_CH;
            const int t = tstage + r;
            float v = 0.0f;
            if (t >= 0 && t < a.T && e0 + e < C) v = a.x[((long)b * a.T + t) * a.ldx + e0 + e];
            Xs[e][r] = v;
        }
        // Ws[k][e][o]: o < 32 the linear column c0 + o, o >= 32 the gate column C + c0 + o - 32
        for (int idx = tid; idx < w * CONV_CH * CONV_BN; idx += 256) {
            const int o = idx % CONV_BN, e = (idx / CONV_BN) % CONV_CH, k = idx / (CONV_CH * CONV_BN);
            const int c = c0 + (o & (GLU_BC - 1));
            float v = 0.0f;
            if (e0 + e < C && c < C) v = a.W[((long)k * C + e0 + e) * n2 + (o < GLU_BC ? c : C + c)];
            Ws[k][e][o] = v;
        }
        __syncthreads();
        const int m = wave * 32 + (lane & 31), kr = lane >> 5;
        for (int k = 0; k < w; ++k) {
#pragma unroll
            for (int cc = 0; cc < CONV_CH; cc += 2) {
                const float av = Xs[cc + kr][m + k];
                const float b0 = Ws[k][cc + kr][lane & 31];
                const float b1 = Ws[k][cc + kr][32 + (lane & 31)];
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc[1], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // C/D layout of v_mfma_f32_32x32x2_f32: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const int c = c0 + (lane & 31);
    if (c >= C) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int t = t0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (t < a.T) glu_store(a, (long)b * a.T + t, c, acc[0][r], acc[1][r]);
    }
}

// scalar kernel: any width
__global__ void convs2s_glu_generic(GluArgs a) {
    const long total = (long)a.B * a.T * a.C;
    const int pad = (a.w - 1) / 2;
    const long n2 = 2L * a.C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % a.C);
        const long bt = i / a.C;
        const int t = (int)(bt % a.T), b = (int)(bt / a.T);
        float lin = 0.0f, gate = 0.0f;
        for (int k = 0; k < a.w; ++k) {
            const int tk = t + k - pad;
            if (tk < 0 || tk >= a.T) continue;
            const float* xr = a.x + ((long)b * a.T + tk) * a.ldx;
            const float* wr = a.W + (long)k * a.C * n2 + c;
            for (int e = 0; e < a.C; ++e) {
                lin = fmaf(xr[e], wr[e * n2], lin);
                gate = fmaf(xr[e], wr[e * n2 + a.C], gate);
            }
        }
        glu_store(a, bt, c, lin, gate);
    }
}

// dz[:, :C] = dy sig; dz[:, C:] = dy lin sig (1 - sig); dx (+)= dy, the residual term (dx may be null)
__global__ void convs2s_glu_dz(const float* __restrict__ dy, long lddy, const float* __restrict__ lin,
                               const float* __restrict__ sig, float* __restrict__ dz, float* __restrict__ dx, long lddx,
                               long rows, int C, int accumulate) {
    const long total = rows * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / C;
        const int c = (int)(i - r * C);
        const float g = dy[r * lddy + c], s = sig[i], l = lin[i];
        dz[r * 2 * C + c] = g * s;
        dz[r * 2 * C + C + c] = g * l * s * (1.0f - s);
        if (dx) dx[r * lddx + c] = accumulate ? dx[r * lddx + c] + g : g;
    }
}

// dbias (+)= the column sums of dz [rows, cols]: conv_bias_grad's fixed order (16 row lanes, added lane by lane)
__global__ __launch_bounds__(BG_COLS * BG_LANES) void convs2s_bias_grad(const float* __restrict__ dz, long rows,
                                                                       int cols, float* dbias, int accumulate) {
    __shared__ float part[BG_LANES][BG_COLS];
    const int cl = threadIdx.x % BG_COLS, lane = threadIdx.x / BG_COLS;
    const int c = blockIdx.x * BG_COLS + cl;
    float v = 0.0f;
    if (c < cols)
        for (long r = lane; r < rows; r += BG_LANES) v += dz[r * cols + c];
    part[lane][cl] = v;
    __syncthreads();
    if (lane != 0 || c >= cols) return;
    v = 0.0f;
    for (int l = 0; l < BG_LANES; ++l) v += part[l][cl];
    dbias[c] = accumulate ? dbias[c] + v : v;
}

static bool glu_ranges_overlap(const float* p, int64_t ldp, const float* q, int64_t ldq, int64_t rows, int64_t cols) {
    const float* pe = p + (rows - 1) * ldp + cols;
    const float* qe = q + (rows - 1) * ldq + cols;
    return !(pe <= q || qe <= p);
}

static int glu_check_sizes(const char* who, int64_t B, int64_t T, int64_t C, int64_t w) {
    NM_REQUIRE(B >= 1 && T >= 1 && C >= 1 && w >= 1, "%s: bad sizes B %lld, T %lld, C %lld, w %lld", who, (long long)B,
               (long long)T, (long long)C, (long long)w);
    NM_REQUIRE(B < (1ll << 31) && T < (1ll << 31) && B * T < (1ll << 31), "%s: B*T = %lld rows beyond 2^31", who,
               (long long)(B * T));
    NM_REQUIRE(C < (1ll << 30) && w < (1ll << 20) && (C + GLU_BC - 1) / GLU_BC <= NM_MAX_GRID_Y &&
                   w * ((C + WG_BM - 1) / WG_BM) * ((2 * C + WG_BN - 1) / WG_BN) < (1ll << 31) &&
                   B * ((T + CONV_BM - 1) / CONV_BM) < (1ll << 31),
               "%s: grid of %lld x %lld workgroups beyond the launch limits", who,
               (long long)(B * ((T + CONV_BM - 1) / CONV_BM)), (long long)((C + GLU_BC - 1) / GLU_BC));
    return NM_OK;
}

extern "C" int nm_conv1d_glu_fwd(void* stream, const float* x, int64_t ldx, int64_t B, int64_t T, int64_t C, int64_t w,
                                 const float* W, const float* bias, float* y, int64_t ldy, float* lin_save,
                                 float* sig_save, int algo) {
    int rc = glu_check_sizes("nm_conv1d_glu_fwd", B, T, C, w);
    if (rc) return rc;
    NM_REQUIRE(x && W && bias && y, "nm_conv1d_glu_fwd: null pointer");
    NM_REQUIRE(ldx >= C, "nm_conv1d_glu_fwd: ldx %lld below C %lld", (long long)ldx, (long long)C);
    NM_REQUIRE(ldy >= C, "nm_conv1d_glu_fwd: ldy %lld below C %lld", (long long)ldy, (long long)C);
    NM_REQUIRE(!glu_ranges_overlap(x, ldx, y, ldy, B * T, C),
               "nm_conv1d_glu_fwd: y aliasing x (a tile reads its neighbours' rows of x as halo)");
    NM_REQUIRE((lin_save == nullptr) == (sig_save == nullptr),
               "nm_conv1d_glu_fwd: lin_save and sig_save come together or not at all");
    NM_REQUIRE(algo >= 0 && algo <= 2, "nm_conv1d_glu_fwd: algo %d (0 auto, 1 mfma, 2 scalar)", algo);
    NM_REQUIRE(algo != 1 || w <= CONV_FAST_MAX_W, "nm_conv1d_glu_fwd: the MFMA kernel takes widths <= %d, not %lld",
               CONV_FAST_MAX_W, (long long)w);
    GluArgs a;
    a.x = x; a.ldx = ldx; a.W = W; a.bias = bias; a.y = y; a.ldy = ldy; a.lin_save = lin_save; a.sig_save = sig_save;
    a.B = (int)B; a.T = (int)T; a.C = (int)C; a.w = (int)w;
    hipStream_t st = nm_stream(stream);
    if (w <= CONV_FAST_MAX_W && algo != 2)
        hipLaunchKernelGGL(convs2s_glu_mfma,
                           dim3((unsigned)(B * ((T + CONV_BM - 1) / CONV_BM)), (unsigned)((C + GLU_BC - 1) / GLU_BC)),
                           dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(convs2s_glu_generic, dim3(ew_grid(B * T * C)), dim3(256), 0, st, a);
    NM_LAUNCH_CHECK("nm_conv1d_glu_fwd");
}

extern "C" int64_t nm_conv1d_glu_workspace_bytes(int64_t B, int64_t T, int64_t C, int64_t w) {
    if (B < 1 || T < 1 || C < 1 || w < 1 || B >= (1ll << 31) || T >= (1ll << 31) || C >= (1ll << 30) || w >= (1ll << 20))
        return 0;
    const int width = (int)w, count = (int)(2 * C);
    return nm_conv1d_wgrad_workspace_bytes((int)B, (int)T, (int)C, 1, &width, &count);
}

extern "C" int nm_conv1d_glu_bwd(void* stream, const float* x, int64_t ldx, int64_t B, int64_t T, int64_t C, int64_t w,
                                 const float* W, const float* lin_save, const float* sig_save, const float* dy,
                                 int64_t lddy, float* dz, float* dx, int64_t lddx, int accumulate_dx, float* dW,
                                 float* dbias, int accumulate_params, void* workspace, int64_t workspace_bytes,
                                 int algo) {
    int rc = glu_check_sizes("nm_conv1d_glu_bwd", B, T, C, w);
    if (rc) return rc;
    NM_REQUIRE(x && W && lin_save && sig_save && dy && dz, "nm_conv1d_glu_bwd: null pointer");
    NM_REQUIRE(ldx >= C, "nm_conv1d_glu_bwd: ldx %lld below C %lld", (long long)ldx, (long long)C);
    NM_REQUIRE(lddy >= C, "nm_conv1d_glu_bwd: lddy %lld below C %lld", (long long)lddy, (long long)C);
    NM_REQUIRE(!dx || lddx >= C, "nm_conv1d_glu_bwd: lddx %lld below C %lld", (long long)lddx, (long long)C);
    NM_REQUIRE(!dx || !glu_ranges_overlap(dx, lddx, dy, lddy, B * T, C), "nm_conv1d_glu_bwd: dx aliasing dy");
    NM_REQUIRE(algo >= 0 && algo <= 2, "nm_conv1d_glu_bwd: algo %d (0 auto, 1 mfma, 2 scalar)", algo);
    NM_REQUIRE(algo != 1 || w <= CONV_FAST_MAX_W, "nm_conv1d_glu_bwd: the MFMA kernels take widths <= %d, not %lld",
               CONV_FAST_MAX_W, (long long)w);
    const int64_t need = nm_conv1d_glu_workspace_bytes(B, T, C, w);
    NM_REQUIRE(!dW || workspace, "nm_conv1d_glu_bwd: the weight gradient needs a workspace");
    NM_REQUIRE(!dW || workspace_bytes >= need, "nm_conv1d_glu_bwd: workspace too small (%lld < %lld bytes)",
               (long long)workspace_bytes, (long long)need);
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.B = (int)B; a.S = (int)T; a.E = (int)C; a.s = 1; a.Sp = (int)T; a.pb = 0;
    a.nw = 1; a.ldp = (int)(2 * C);
    a.wd[0].W = W; a.wd[0].w = (int)w; a.wd[0].n = (int)(2 * C); a.wd[0].col = 0;
    a.x = x; a.ldx = ldx; a.dz = dz; a.dx = dx; a.lddx = lddx; a.accumulate = 1;     // onto the residual term
    const bool mfma = w <= CONV_FAST_MAX_W && algo != 2;
    hipStream_t st = nm_stream(stream);
    hipLaunchKernelGGL(convs2s_glu_dz, dim3(ew_grid(B * T * C)), dim3(256), 0, st, dy, (long)lddy, lin_save, sig_save,
                       dz, dx, (long)lddx, (long)(B * T), (int)C, accumulate_dx);
    float* const dW_tab[1] = {dW};
    conv_grads_launch(st, a, mfma, dW ? dW_tab : nullptr, need, workspace, accumulate_params);
    if (dbias)
        hipLaunchKernelGGL(convs2s_bias_grad, dim3((unsigned)((2 * C + BG_COLS - 1) / BG_COLS)),
                           dim3(BG_COLS * BG_LANES), 0, st, dz, (long)(B * T), (int)(2 * C), dbias, accumulate_params);
    NM_LAUNCH_CHECK("nm_conv1d_glu_bwd");
}
