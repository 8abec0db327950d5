// The image stack (include/nmhip_image.h): the device work of encoders/cnn_encoder.py -- tf.layers.conv2d at stride 1,
// tf.layers.batch_normalization (+ ReLU), tf.layers.max_pooling2d / average_pooling2d.  Maps are NHWC with a leading
// dimension, filters TensorFlow's [k, k, Cin, Cout].
//
//   img2d_conv_mfma          implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32), the anatomy of convs2s_glu_mfma in
//                            nm_conv.hip: a 2-D convolution is the sum over the k filter rows of 1-D convolutions along
//                            W, so a workgroup owns 128 positions of ONE output row x 64 output channels; per chunk of 16
//                            input channels and per filter row it stages the input row's 128 + k - 1 positions (halo
//                            included) once and reads them shifted for every tap of that row.  The data gradient is the
//                            same kernel over dy with the filter read flipped and transposed (ConvArgs::flip).
//   img2d_conv_scalar        one thread per output value, any k; same flip switch.
//   img2d_conv_wgrad_mfma    dW as a product over positions: a wave owns a 32 x 32 tile of one tap's [Cin, Cout] and one
//                            slice of the positions; both operands come straight from global memory (32 adjacent
//                            channels per half wave).  Slabs go to the workspace.
//   img2d_conv_wgrad_scalar  one thread per (slice, filter or bias element); the bias slabs of both algos.
//   img2d_conv_wgrad_sum     the slices added one after the other: the fixed order that makes two runs bit-equal.
//   img2d_bn_stats           one workgroup of 32 channels x 32 row lanes: the mean, then the squared deviations from it
//                            (two passes, never E[x^2] - E[x]^2), summed in double, LDS partials added in lane order;
//                            moving statistics.
//   img2d_bn_apply           normalise, scale, shift, ReLU -- training (batch statistics) and inference (moving ones).
//   img2d_bn_bwd_sums / img2d_bn_bwd_dx   the two channel sums, then the input gradient.
//   img2d_window_fwd / img2d_window_bwd   pooling windows; the gradient is a gather over the windows that hold a position.
//   img2d_columns            the transpose that turns a map into the sequence of its columns, and back.
// No floating-point atomics anywhere.
#include "nm_common.h"
#include "../../include/nmhip_image.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// TensorFlow 1.x takes the fused kernel for 4-D input, and what that kernel hands to the moving-variance update is the
// UNBIASED batch variance (rows / (rows - 1)), while the normalisation uses the biased one.  This rests on reading
// TensorFlow's source, not on a run of it; false: the biased variance enters the moving variance.
constexpr bool BN_MOVING_VARIANCE_UNBIASED = true;

constexpr int IMG_BM = 128;          // positions (along W) of a workgroup tile
constexpr int IMG_BN = 64;           // output channels of a workgroup tile
constexpr int IMG_CH = 16;           // input channels staged at a time
constexpr int IMG_MFMA_MAX_K = 7;    // widest filter the matrix-core kernels stage
constexpr int IMG_XR = IMG_BM + IMG_MFMA_MAX_K - 1 + 2;   // staged positions of a row (+2: rows of a half wave apart in banks)
constexpr int IMG_SLICE = 128;       // positions of a weight-gradient slice, at least
constexpr int IMG_MAX_SLICES = 256;

struct ConvArgs {
    const float* x;          // [B, IH, IW, Cin] rows of ldx
    long ldx;
    const float* W;          // the forward filter [k, k, ., .]
    const float* bias;       // [Cout] or null
    float* y;                // [B, OH, OW, Cout] rows of ldy
    long ldy;
    int B, IH, IW, Cin, OH, OW, Cout, k, pt, pl;
    int flip;                // 0: W[ky][kx][ci][co].  1 (data gradient; Cin is the forward Cout): W[k-1-ky][k-1-kx][co][ci]
    int accumulate;
};

__device__ __forceinline__ float conv_w(const ConvArgs& a, int ky, int kx, int ci, int co) {
    if (a.flip) return a.W[(((long)(a.k - 1 - ky) * a.k + (a.k - 1 - kx)) * a.Cout + co) * a.Cin + ci];
    return a.W[(((long)ky * a.k + kx) * a.Cin + ci) * a.Cout + co];
}

__global__ __launch_bounds__(256) void img2d_conv_mfma(ConvArgs a) {
    __shared__ float Xs[IMG_CH][IMG_XR];                           // [channel][position of the staged row]
    __shared__ float Ws[IMG_MFMA_MAX_K][IMG_CH][IMG_BN];           // [kx][channel][output channel]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles_w = (a.OW + IMG_BM - 1) / IMG_BM;
    const int ox0 = (blockIdx.x % tiles_w) * IMG_BM;
    const int oy = (blockIdx.x / tiles_w) % a.OH;
    const int b = blockIdx.x / (tiles_w * a.OH);
    const int c0 = blockIdx.y * IMG_BN;
    const int k = a.k, ncols = IMG_BM + k - 1;

    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;

    for (int e0 = 0; e0 < a.Cin; e0 += IMG_CH) {
        for (int ky = 0; ky < k; ++ky) {
            const int iy = oy + ky - a.pt;                         // the same for the whole workgroup
            if (iy < 0 || iy >= a.IH) continue;
            const float* xrow = a.x + ((long)b * a.IH + iy) * a.IW * a.ldx;
            for (int idx = tid; idx < IMG_CH * ncols; idx += 256) {
                const int e = idx % IMG_CH, r = idx / IMG_CH;
                const int ix = ox0 - a.pl + r;
                float v = 0.0f;
                if (ix >= 0 && ix < a.IW && e0 + e < a.Cin) v = xrow[(long)ix * a.ldx + e0 + e];
                Xs[e][r] = v;
            }
            for (int idx = tid; idx < k * IMG_CH * IMG_BN; idx += 256) {
                const int o = idx % IMG_BN, e = (idx / IMG_BN) % IMG_CH, kx = idx / (IMG_CH * IMG_BN);
                float v = 0.0f;
                if (e0 + e < a.Cin && c0 + o < a.Cout) v = conv_w(a, ky, kx, e0 + e, c0 + o);
                Ws[kx][e][o] = v;
            }
            __syncthreads();
            const int m = wave * 32 + (lane & 31), kr = lane >> 5;
            for (int kx = 0; kx < k; ++kx) {
#pragma unroll
                for (int cc = 0; cc < IMG_CH; cc += 2) {
                    const float av = Xs[cc + kr][m + kx];
                    const float b0 = Ws[kx][cc + kr][lane & 31];
                    const float b1 = Ws[kx][cc + kr][32 + (lane & 31)];
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc[1], 0, 0, 0);
                }
            }
            __syncthreads();
        }
    }

    // C/D layout of v_mfma_f32_32x32x2_f32: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    float* yrow = a.y + ((long)b * a.OH + oy) * a.OW * a.ldy;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int co = c0 + j * 32 + (lane & 31);
        if (co >= a.Cout) continue;
        const float bv = a.bias ? a.bias[co] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ox = ox0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (ox >= a.OW) continue;
            float* out = yrow + (long)ox * a.ldy + co;
            const float v = acc[j][r] + bv;
            *out = a.accumulate ? *out + v : v;
        }
    }
}

__global__ __launch_bounds__(256) void img2d_conv_scalar(ConvArgs a) {
    const long total = (long)a.B * a.OH * a.OW * a.Cout;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int co = (int)(i % a.Cout);
        const long p = i / a.Cout;
        const int ox = (int)(p % a.OW), oy = (int)((p / a.OW) % a.OH), b = (int)(p / ((long)a.OW * a.OH));
        float acc = 0.0f;
        for (int ky = 0; ky < a.k; ++ky) {
            const int iy = oy + ky - a.pt;
            if (iy < 0 || iy >= a.IH) continue;
            for (int kx = 0; kx < a.k; ++kx) {
                const int ix = ox + kx - a.pl;
                if (ix < 0 || ix >= a.IW) continue;
                const float* xr = a.x + (((long)b * a.IH + iy) * a.IW + ix) * a.ldx;
                for (int ci = 0; ci < a.Cin; ++ci) acc = fmaf(xr[ci], conv_w(a, ky, kx, ci, co), acc);
            }
        }
        if (a.bias) acc += a.bias[co];
        float* out = a.y + p * a.ldy + co;
        *out = a.accumulate ? *out + acc : acc;
    }
}

// ---- filter and bias gradients ---------------------------------------------------------------------------------------------
struct WgradArgs {
    const float* x;          // [B, H, W, Cin] rows of ldx
    long ldx;
    const float* dy;         // [B, OH, OW, Cout] rows of lddy
    long lddy;
    float* ws;               // [slices][k*k*Cin*Cout + Cout]
    int B, H, W, Cin, OH, OW, Cout, k, pt, pl;
    long P;                  // B*OH*OW positions
    long chunk;              // positions of a slice
    int slices;
};

__device__ __forceinline__ long wgrad_slab(const WgradArgs& a) { return (long)a.k * a.k * a.Cin * a.Cout + a.Cout; }

// the input value that output position p meets under tap (ky, kx), channel ci; zero outside the map
__device__ __forceinline__ float wgrad_x(const WgradArgs& a, long p, int ky, int kx, int ci) {
    const int ox = (int)(p % a.OW), oy = (int)((p / a.OW) % a.OH);
    const long b = p / ((long)a.OW * a.OH);
    const int iy = oy + ky - a.pt, ix = ox + kx - a.pl;
    if (iy < 0 || iy >= a.H || ix < 0 || ix >= a.W) return 0.0f;
    return a.x[((b * a.H + iy) * a.W + ix) * a.ldx + ci];
}

// elements [lo, hi) of every slice's slab: below k*k*Cin*Cout a filter element, above it a bias element
__global__ __launch_bounds__(256) void img2d_conv_wgrad_scalar(WgradArgs a, long lo, long hi) {
    const long nw = (long)a.k * a.k * a.Cin * a.Cout, slab = wgrad_slab(a), span = hi - lo;
    const long total = span * a.slices;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long e = lo + i % span;
        const int s = (int)(i / span);
        const long p0 = s * a.chunk, p1 = p0 + a.chunk < a.P ? p0 + a.chunk : a.P;
        float acc = 0.0f;
        if (e >= nw) {
            const int co = (int)(e - nw);
            for (long p = p0; p < p1; ++p) acc += a.dy[p * a.lddy + co];
        } else {
            const int co = (int)(e % a.Cout), ci = (int)((e / a.Cout) % a.Cin);
            const int tap = (int)(e / ((long)a.Cout * a.Cin)), ky = tap / a.k, kx = tap % a.k;
            for (long p = p0; p < p1; ++p) acc = fmaf(wgrad_x(a, p, ky, kx, ci), a.dy[p * a.lddy + co], acc);
        }
        a.ws[s * slab + e] = acc;
    }
}

// blockIdx.x: (tap, tile of 32 input channels, tile of 32 output channels); blockIdx.y: slice.  One wave.
__global__ __launch_bounds__(64) void img2d_conv_wgrad_mfma(WgradArgs a) {
    const int lane = threadIdx.x, kr = lane >> 5, l32 = lane & 31;
    const int tiles_o = (a.Cout + 31) / 32, tiles_i = (a.Cin + 31) / 32;
    const int to = blockIdx.x % tiles_o, ti = (blockIdx.x / tiles_o) % tiles_i, tap = blockIdx.x / (tiles_o * tiles_i);
    const int ky = tap / a.k, kx = tap % a.k;
    const int ci = ti * 32 + l32, co = to * 32 + l32;
    const int s = blockIdx.y;
    const long p0 = s * a.chunk, p1 = p0 + a.chunk < a.P ? p0 + a.chunk : a.P;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (long p = p0; p < p1; p += 2) {
        const long pp = p + kr;
        float av = 0.0f, bv = 0.0f;
        if (pp < p1) {
            if (ci < a.Cin) av = wgrad_x(a, pp, ky, kx, ci);
            if (co < a.Cout) bv = a.dy[pp * a.lddy + co];
        }
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
    }
    if (co >= a.Cout) return;
    float* slab = a.ws + s * wgrad_slab(a) + (long)tap * a.Cin * a.Cout;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = ti * 32 + (r & 3) + 8 * (r >> 2) + 4 * kr;
        if (row < a.Cin) slab[(long)row * a.Cout + co] = acc[r];
    }
}

// out[e] (+)= ws[0][lo + e] + ws[1][lo + e] + ... in that order
__global__ __launch_bounds__(256) void img2d_conv_wgrad_sum(const float* __restrict__ ws, long slab, int slices, long lo,
                                                            long n, float* __restrict__ out, int accumulate) {
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        float v = 0.0f;
        for (int s = 0; s < slices; ++s) v += ws[s * slab + lo + e];
        out[e] = accumulate ? out[e] + v : v;
    }
}

// ---- batch normalisation -----------------------------------------------------------------------------------------------------
constexpr int BN_COLS = 32, BN_LANES = 32;

// the channel sums of f(row, channel) over the rows, accumulated in double (these kernels wait for memory, and the sums
// of 10^5 rows feed a difference of nearly equal numbers in the backward pass), lane partials added in lane order; every
// thread of the workgroup calls it, the result is valid where lane == 0
template <typename F>
__device__ __forceinline__ double bn_colsum(double (*part)[BN_COLS + 1], long rows, int c, int C, F f) {
    const int cl = threadIdx.x, lane = threadIdx.y;
    double v = 0.0;
    if (c < C)
        for (long r = lane; r < rows; r += BN_LANES) v += (double)f(r);
    __syncthreads();                                               // the previous use of part is over
    part[lane][cl] = v;
    __syncthreads();
    double sum = 0.0;
    if (lane == 0)
        for (int l = 0; l < BN_LANES; ++l) sum += part[l][cl];
    return sum;
}

__global__ __launch_bounds__(BN_COLS * BN_LANES) void img2d_bn_stats(
    const float* __restrict__ x, long ldx, long rows, int C, float momentum, float* moving_mean, float* moving_var,
    float* __restrict__ batch_mean, float* __restrict__ batch_var) {
    __shared__ double part[BN_LANES][BN_COLS + 1];
    __shared__ float smean[BN_COLS];
    const int c = blockIdx.x * BN_COLS + threadIdx.x;
    const float* xc = x + c;
    const double sum = bn_colsum(part, rows, c, C, [&](long r) { return xc[r * ldx]; });
    if (threadIdx.y == 0) smean[threadIdx.x] = (float)(sum / (double)rows);
    __syncthreads();
    const float mean = smean[threadIdx.x];                         // the rounded mean: what the normalisation subtracts
    const double sq = bn_colsum(part, rows, c, C, [&](long r) { const float d = xc[r * ldx] - mean; return d * d; });
    if (threadIdx.y != 0 || c >= C) return;
    const float var = (float)(sq / (double)rows);
    batch_mean[c] = mean;
    batch_var[c] = var;
    if (moving_mean) {
        const float fed = BN_MOVING_VARIANCE_UNBIASED ? var * ((float)rows / (float)(rows > 1 ? rows - 1 : 1)) : var;
        moving_mean[c] = momentum * moving_mean[c] + (1.0f - momentum) * mean;
        moving_var[c] = momentum * moving_var[c] + (1.0f - momentum) * fed;
    }
}

__global__ __launch_bounds__(256) void img2d_bn_apply(const float* __restrict__ x, long ldx, long rows, int C,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      const float* __restrict__ mean, const float* __restrict__ var,
                                                      float eps, int relu, float* __restrict__ y, long ldy) {
    const long total = rows * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / C;
        const int c = (int)(i - r * C);
        const float rstd = 1.0f / sqrtf(var[c] + eps);
        float v = (x[r * ldx + c] - mean[c]) * rstd * gamma[c] + beta[c];
        if (relu) v = fmaxf(v, 0.0f);
        y[r * ldy + c] = v;
    }
}

__global__ __launch_bounds__(BN_COLS * BN_LANES) void img2d_bn_bwd_sums(
    const float* __restrict__ x, long ldx, const float* __restrict__ y, long ldy, const float* __restrict__ dy, long lddy,
    long rows, int C, const float* __restrict__ mean, const float* __restrict__ var, float eps, int relu,
    float* __restrict__ sums, float* dgamma, float* dbeta, int accumulate) {
    __shared__ double part[BN_LANES][BN_COLS + 1];
    const int c = blockIdx.x * BN_COLS + threadIdx.x;
    const float m = c < C ? mean[c] : 0.0f;
    const float rstd = c < C ? 1.0f / sqrtf(var[c] + eps) : 0.0f;
    auto g = [&](long r) { return (!relu || y[r * ldy + c] > 0.0f) ? dy[r * lddy + c] : 0.0f; };
    const float s1 = (float)bn_colsum(part, rows, c, C, g);
    const float s2 = (float)bn_colsum(part, rows, c, C, [&](long r) { return g(r) * ((x[r * ldx + c] - m) * rstd); });
    if (threadIdx.y != 0 || c >= C) return;
    sums[c] = s1;
    sums[C + c] = s2;
    if (dbeta) dbeta[c] = accumulate ? dbeta[c] + s1 : s1;
    if (dgamma) dgamma[c] = accumulate ? dgamma[c] + s2 : s2;
}

__global__ __launch_bounds__(256) void img2d_bn_bwd_dx(
    const float* __restrict__ x, long ldx, const float* __restrict__ y, long ldy, const float* dy, long lddy, long rows,
    int C, const float* __restrict__ gamma, const float* __restrict__ mean, const float* __restrict__ var, float eps,
    int relu, const float* __restrict__ sums, float* dx, long lddx, int accumulate) {
    const long total = rows * C;
    const float inv = 1.0f / (float)rows;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / C;
        const int c = (int)(i - r * C);
        const float rstd = 1.0f / sqrtf(var[c] + eps);
        const float xhat = (x[r * ldx + c] - mean[c]) * rstd;
        const float g = (!relu || y[r * ldy + c] > 0.0f) ? dy[r * lddy + c] : 0.0f;
        const float v = gamma[c] * rstd * (g - sums[c] * inv - xhat * (sums[C + c] * inv));
        float* out = dx + r * lddx + c;
        *out = accumulate ? *out + v : v;
    }
}

// ---- pooling windows -----------------------------------------------------------------------------------------------------------
struct WindowArgs {
    int B, H, W, C, OH, OW, kh, kw, sh, sw, pt, pl, mode;
};

__global__ __launch_bounds__(256) void img2d_window_fwd(WindowArgs a, const float* __restrict__ x, long ldx,
                                                        float* __restrict__ y, long ldy, int32_t* __restrict__ argmax) {
    const long total = (long)a.B * a.OH * a.OW * a.C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % a.C);
        const long p = i / a.C;
        const int ox = (int)(p % a.OW), oy = (int)((p / a.OW) % a.OH);
        const long b = p / ((long)a.OW * a.OH);
        const int y0 = oy * a.sh - a.pt, x0 = ox * a.sw - a.pl;
        float best = -INFINITY, sum = 0.0f;
        int where = -1, count = 0;
        for (int ky = 0; ky < a.kh; ++ky) {
            const int iy = y0 + ky;
            if (iy < 0 || iy >= a.H) continue;
            for (int kx = 0; kx < a.kw; ++kx) {
                const int ix = x0 + kx;
                if (ix < 0 || ix >= a.W) continue;
                const float v = x[((b * a.H + iy) * a.W + ix) * ldx + c];
                if (where < 0 || v > best) { best = v; where = iy * a.W + ix; }       // strictly greater: the first maximum stays
                sum += v;
                ++count;
            }
        }
        y[p * ldy + c] = a.mode == NM_WINDOW_MAX ? best : sum / (float)count;
        if (argmax) argmax[i] = where;
    }
}

__device__ __forceinline__ int window_inside(int o, int stride, int pad, int k, int n) {
    const int lo = o * stride - pad, hi = lo + k;
    return (hi < n ? hi : n) - (lo > 0 ? lo : 0);
}

__global__ __launch_bounds__(256) void img2d_window_bwd(WindowArgs a, const float* __restrict__ dy, long lddy,
                                                        const int32_t* __restrict__ argmax, float* __restrict__ dx,
                                                        long lddx, int accumulate) {
    const long total = (long)a.B * a.H * a.W * a.C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % a.C);
        const long p = i / a.C;
        const int ix = (int)(p % a.W), iy = (int)((p / a.W) % a.H);
        const long b = p / ((long)a.W * a.H);
        // windows oy with oy*sh - pt <= iy < oy*sh - pt + kh
        int oy_lo = iy + a.pt - a.kh + 1;
        oy_lo = oy_lo <= 0 ? 0 : (oy_lo + a.sh - 1) / a.sh;
        int oy_hi = (iy + a.pt) / a.sh;
        if (oy_hi >= a.OH) oy_hi = a.OH - 1;
        int ox_lo = ix + a.pl - a.kw + 1;
        ox_lo = ox_lo <= 0 ? 0 : (ox_lo + a.sw - 1) / a.sw;
        int ox_hi = (ix + a.pl) / a.sw;
        if (ox_hi >= a.OW) ox_hi = a.OW - 1;
        const int me = iy * a.W + ix;
        float v = 0.0f;
        for (int oy = oy_lo; oy <= oy_hi; ++oy)
            for (int ox = ox_lo; ox <= ox_hi; ++ox) {
                const long q = (b * a.OH + oy) * a.OW + ox;
                if (a.mode == NM_WINDOW_MAX) {
                    if (argmax[q * a.C + c] == me) v += dy[q * lddy + c];
                } else {
                    const int n = window_inside(oy, a.sh, a.pt, a.kh, a.H) * window_inside(ox, a.sw, a.pl, a.kw, a.W);
                    v += dy[q * lddy + c] / (float)n;
                }
            }
        float* out = dx + p * lddx + c;
        *out = accumulate ? *out + v : v;
    }
}

// ---- a map as the sequence of its columns ----------------------------------------------------------------------------------------
// cols[b, x, y*C + c] <-> map[b, y, x, c]; one thread per element, indexed in the order of what it WRITES
__global__ __launch_bounds__(256) void img2d_columns(const float* __restrict__ src, float* __restrict__ dst, long B, int H,
                                                     int W, int C, int inverse) {
    const long total = B * H * W * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        long r = i / C;
        int x, y;
        if (inverse) { x = (int)(r % W); r /= W; y = (int)(r % H); }       // i walks the map
        else { y = (int)(r % H); r /= H; x = (int)(r % W); }               // i walks the columns
        const long b = r / (inverse ? H : W);
        const long in_map = ((b * H + y) * W + x) * C + c, in_cols = ((b * W + x) * H + y) * C + c;
        if (inverse) dst[in_map] = src[in_cols];
        else dst[in_cols] = src[in_map];
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
constexpr int64_t IMG_MAX_ELEMS = (1ll << 31) - 1;

unsigned ew_blocks(int64_t total) {
    const int64_t blocks = (total + 255) / 256;
    return (unsigned)(blocks < 1 ? 1 : (blocks > (1 << 20) ? (1 << 20) : blocks));
}

bool ranges_overlap(const float* p, int64_t ldp, int64_t prows, int64_t pcols, const float* q, int64_t ldq, int64_t qrows,
                    int64_t qcols) {
    const float* pe = p + (prows - 1) * ldp + pcols;
    const float* qe = q + (qrows - 1) * ldq + qcols;
    return !(pe <= q || qe <= p);
}

struct ConvShape {
    int64_t OH, OW, pt, pl, P, slices, chunk, slab;
};

int conv_shape(const char* who, int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t k, int64_t Cout, int padding,
               ConvShape* s) {
    NM_REQUIRE(B >= 1 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1 && k >= 1,
               "%s: bad sizes B %lld, H %lld, W %lld, Cin %lld, Cout %lld, k %lld", who, (long long)B, (long long)H,
               (long long)W, (long long)Cin, (long long)Cout, (long long)k);
    NM_REQUIRE(padding == NM_PAD_VALID || padding == NM_PAD_SAME, "%s: padding %d (0 VALID, 1 SAME)", who, padding);
    NM_REQUIRE(padding == NM_PAD_SAME || (H >= k && W >= k), "%s: VALID padding with a %lld x %lld map below the %lld x %lld filter",
               who, (long long)H, (long long)W, (long long)k, (long long)k);
    NM_REQUIRE(B <= IMG_MAX_ELEMS && H <= IMG_MAX_ELEMS && W <= IMG_MAX_ELEMS && Cin <= IMG_MAX_ELEMS &&
                   Cout <= IMG_MAX_ELEMS && k <= 1024,
               "%s: a size beyond 2^31 - 1 (k beyond 1024)", who);
    s->OH = padding == NM_PAD_SAME ? H : H - k + 1;
    s->OW = padding == NM_PAD_SAME ? W : W - k + 1;
    s->pt = s->pl = padding == NM_PAD_SAME ? (k - 1) / 2 : 0;
    const int64_t mx = Cin > Cout ? Cin : Cout;
    NM_REQUIRE(B * H <= IMG_MAX_ELEMS && B * H * W <= IMG_MAX_ELEMS && (double)B * H * W * mx <= (double)IMG_MAX_ELEMS &&
                   (double)k * k * Cin * Cout <= (double)IMG_MAX_ELEMS,
               "%s: a map or the filter holds more than 2^31 - 1 elements", who);
    s->P = B * s->OH * s->OW;
    s->slices = (s->P + IMG_SLICE - 1) / IMG_SLICE;
    if (s->slices > IMG_MAX_SLICES) s->slices = IMG_MAX_SLICES;
    s->chunk = (s->P + s->slices - 1) / s->slices;
    s->slices = (s->P + s->chunk - 1) / s->chunk;
    s->slab = k * k * Cin * Cout + Cout;
    return NM_OK;
}

// algo 0: the matrix-core kernel where tools/bench_conv2d.py measured it faster: rows long
// enough to fill a good part of a 128-position tile and enough input channels to feed the 16-channel chunks
bool conv_auto_mfma(int64_t ow, int64_t cin, int64_t k) { return k <= IMG_MFMA_MAX_K && ow >= 32 && cin >= 8; }

int conv_launch(const char* who, hipStream_t st, const ConvArgs& a, bool mfma) {
    if (mfma) {
        const int64_t gx = (int64_t)a.B * a.OH * ((a.OW + IMG_BM - 1) / IMG_BM), gy = (a.Cout + IMG_BN - 1) / IMG_BN;
        NM_REQUIRE(gx <= IMG_MAX_ELEMS && gy <= NM_MAX_GRID_Y, "%s: grid of %lld x %lld workgroups beyond the launch limits",
                   who, (long long)gx, (long long)gy);
        hipLaunchKernelGGL(img2d_conv_mfma, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL(img2d_conv_scalar, dim3(ew_blocks((int64_t)a.B * a.OH * a.OW * a.Cout)), dim3(256), 0, st, a);
    }
    NM_LAUNCH_CHECK(who);
}

int window_shape(const char* who, int64_t B, int64_t H, int64_t W, int64_t C, int64_t kh, int64_t kw, int64_t sh,
                 int64_t sw, int padding, int mode, WindowArgs* a) {
    NM_REQUIRE(B >= 1 && H >= 1 && W >= 1 && C >= 1, "%s: bad sizes B %lld, H %lld, W %lld, C %lld", who, (long long)B,
               (long long)H, (long long)W, (long long)C);
    NM_REQUIRE(kh >= 1 && kw >= 1 && sh >= 1 && sw >= 1, "%s: bad window %lld x %lld, stride %lld x %lld", who,
               (long long)kh, (long long)kw, (long long)sh, (long long)sw);
    NM_REQUIRE(padding == NM_PAD_VALID || padding == NM_PAD_SAME, "%s: padding %d (0 VALID, 1 SAME)", who, padding);
    NM_REQUIRE(mode == NM_WINDOW_MAX || mode == NM_WINDOW_AVG, "%s: mode %d (0 max, 1 average)", who, mode);
    NM_REQUIRE(padding == NM_PAD_SAME || (H >= kh && W >= kw), "%s: VALID padding with a %lld x %lld map below the %lld x %lld window",
               who, (long long)H, (long long)W, (long long)kh, (long long)kw);
    NM_REQUIRE(B <= IMG_MAX_ELEMS && H <= IMG_MAX_ELEMS && W <= IMG_MAX_ELEMS && C <= IMG_MAX_ELEMS &&
                   kh <= IMG_MAX_ELEMS && kw <= IMG_MAX_ELEMS && sh <= IMG_MAX_ELEMS && sw <= IMG_MAX_ELEMS &&
                   B * H <= IMG_MAX_ELEMS && B * H * W <= IMG_MAX_ELEMS && (double)B * H * W * C <= (double)IMG_MAX_ELEMS,
               "%s: a map holds more than 2^31 - 1 elements", who);
    int64_t oh, ow, pt = 0, pl = 0;
    if (padding == NM_PAD_SAME) {
        oh = (H + sh - 1) / sh;
        ow = (W + sw - 1) / sw;
        const int64_t ph = (oh - 1) * sh + kh - H, pw = (ow - 1) * sw + kw - W;
        pt = ph > 0 ? ph / 2 : 0;
        pl = pw > 0 ? pw / 2 : 0;
    } else {
        oh = (H - kh) / sh + 1;
        ow = (W - kw) / sw + 1;
    }
    a->B = (int)B; a->H = (int)H; a->W = (int)W; a->C = (int)C; a->OH = (int)oh; a->OW = (int)ow;
    a->kh = (int)kh; a->kw = (int)kw; a->sh = (int)sh; a->sw = (int)sw; a->pt = (int)pt; a->pl = (int)pl; a->mode = mode;
    return NM_OK;
}

int bn_check(const char* who, int64_t rows, int64_t C) {
    NM_REQUIRE(rows >= 1 && C >= 1, "%s: bad sizes rows %lld, C %lld", who, (long long)rows, (long long)C);
    NM_REQUIRE(rows <= IMG_MAX_ELEMS && C <= IMG_MAX_ELEMS && rows * C <= IMG_MAX_ELEMS,
               "%s: rows * C = %lld elements beyond 2^31 - 1", who, (long long)(rows * C));
    return NM_OK;
}

}  // namespace

extern "C" int nm_conv2d_fwd(void* stream, const float* x, int64_t ldx, int64_t B, int64_t H, int64_t W, int64_t Cin,
                             const float* filt, int64_t k, int64_t Cout, int padding, const float* bias, float* y,
                             int64_t ldy, int algo) {
    ConvShape s;
    int rc = conv_shape("nm_conv2d_fwd", B, H, W, Cin, k, Cout, padding, &s);
    if (rc) return rc;
    NM_REQUIRE(x && filt && bias && y, "nm_conv2d_fwd: null pointer");
    NM_REQUIRE(ldx >= Cin, "nm_conv2d_fwd: ldx %lld below Cin %lld", (long long)ldx, (long long)Cin);
    NM_REQUIRE(ldy >= Cout, "nm_conv2d_fwd: ldy %lld below Cout %lld", (long long)ldy, (long long)Cout);
    NM_REQUIRE((double)B * H * W * ldx < 9e18 && (double)s.P * ldy < 9e18, "nm_conv2d_fwd: leading dimension too large");
    NM_REQUIRE(!ranges_overlap(x, ldx, B * H * W, Cin, y, ldy, s.P, Cout), "nm_conv2d_fwd: y overlapping x");
    NM_REQUIRE(algo >= 0 && algo <= 2, "nm_conv2d_fwd: algo %d (0 auto, 1 mfma, 2 scalar)", algo);
    NM_REQUIRE(algo != 1 || k <= IMG_MFMA_MAX_K, "nm_conv2d_fwd: the MFMA kernel takes k <= %d, not %lld", IMG_MFMA_MAX_K,
               (long long)k);
    ConvArgs a;
    a.x = x; a.ldx = ldx; a.W = filt; a.bias = bias; a.y = y; a.ldy = ldy;
    a.B = (int)B; a.IH = (int)H; a.IW = (int)W; a.Cin = (int)Cin; a.OH = (int)s.OH; a.OW = (int)s.OW; a.Cout = (int)Cout;
    a.k = (int)k; a.pt = (int)s.pt; a.pl = (int)s.pl; a.flip = 0; a.accumulate = 0;
    return conv_launch("nm_conv2d_fwd", nm_stream(stream), a, algo == 1 || (algo == 0 && conv_auto_mfma(s.OW, Cin, k)));
}

extern "C" int64_t nm_conv2d_workspace_bytes(int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t k, int64_t Cout,
                                             int padding) {
    ConvShape s;
    if (conv_shape("nm_conv2d_workspace_bytes", B, H, W, Cin, k, Cout, padding, &s)) return 0;
    return s.slices * s.slab * (int64_t)sizeof(float);
}

extern "C" int nm_conv2d_bwd(void* stream, const float* x, int64_t ldx, int64_t B, int64_t H, int64_t W, int64_t Cin,
                             const float* filt, int64_t k, int64_t Cout, int padding, const float* dy, int64_t lddy,
                             float* dx, int64_t lddx, int accumulate_dx, float* dfilt, float* dbias,
                             int accumulate_params, void* workspace, int64_t workspace_bytes, int algo) {
    ConvShape s;
    int rc = conv_shape("nm_conv2d_bwd", B, H, W, Cin, k, Cout, padding, &s);
    if (rc) return rc;
    NM_REQUIRE(x && filt && dy, "nm_conv2d_bwd: null pointer");
    NM_REQUIRE(ldx >= Cin, "nm_conv2d_bwd: ldx %lld below Cin %lld", (long long)ldx, (long long)Cin);
    NM_REQUIRE(lddy >= Cout, "nm_conv2d_bwd: lddy %lld below Cout %lld", (long long)lddy, (long long)Cout);
    NM_REQUIRE(!dx || lddx >= Cin, "nm_conv2d_bwd: lddx %lld below Cin %lld", (long long)lddx, (long long)Cin);
    NM_REQUIRE((double)B * H * W * ldx < 9e18 && (double)s.P * lddy < 9e18 && (double)B * H * W * lddx < 9e18,
               "nm_conv2d_bwd: leading dimension too large");
    NM_REQUIRE(!dx || !ranges_overlap(dx, lddx, B * H * W, Cin, dy, lddy, s.P, Cout), "nm_conv2d_bwd: dx overlapping dy");
    NM_REQUIRE(algo >= 0 && algo <= 2, "nm_conv2d_bwd: algo %d (0 auto, 1 mfma, 2 scalar)", algo);
    NM_REQUIRE(algo != 1 || k <= IMG_MFMA_MAX_K, "nm_conv2d_bwd: the MFMA kernels take k <= %d, not %lld", IMG_MFMA_MAX_K,
               (long long)k);
    const int64_t need = s.slices * s.slab * (int64_t)sizeof(float);
    if (dfilt || dbias) {
        NM_REQUIRE(workspace, "nm_conv2d_bwd: the filter and bias gradients need a workspace");
        if (workspace_bytes < need)
            NM_FAIL(NM_ERR_WORKSPACE, "nm_conv2d_bwd: workspace too small (%lld < %lld bytes)", (long long)workspace_bytes,
                    (long long)need);
    }
    hipStream_t st = nm_stream(stream);
    if (dx) {
        // the transposed convolution: over dy [B, OH, OW, Cout] with the filter flipped, padded by k - 1 - pad
        ConvArgs a;
        a.x = dy; a.ldx = lddy; a.W = filt; a.bias = nullptr; a.y = dx; a.ldy = lddx;
        a.B = (int)B; a.IH = (int)s.OH; a.IW = (int)s.OW; a.Cin = (int)Cout; a.OH = (int)H; a.OW = (int)W; a.Cout = (int)Cin;
        a.k = (int)k; a.pt = (int)(k - 1 - s.pt); a.pl = (int)(k - 1 - s.pl); a.flip = 1; a.accumulate = accumulate_dx != 0;
        rc = conv_launch("nm_conv2d_bwd", st, a, algo == 1 || (algo == 0 && conv_auto_mfma(W, Cout, k)));
        if (rc) return rc;
    }
    if (!dfilt && !dbias) return NM_OK;
    WgradArgs g;
    g.x = x; g.ldx = ldx; g.dy = dy; g.lddy = lddy; g.ws = static_cast<float*>(workspace);
    g.B = (int)B; g.H = (int)H; g.W = (int)W; g.Cin = (int)Cin; g.OH = (int)s.OH; g.OW = (int)s.OW; g.Cout = (int)Cout;
    g.k = (int)k; g.pt = (int)s.pt; g.pl = (int)s.pl; g.P = s.P; g.chunk = s.chunk; g.slices = (int)s.slices;
    const int64_t nw = s.slab - Cout;
    const bool mfma = algo == 1 || (algo == 0 && conv_auto_mfma(s.OW, Cin, k) && Cout >= 8);
    if (dfilt) {
        if (mfma) {
            const int64_t gx = k * k * ((Cin + 31) / 32) * ((Cout + 31) / 32);
            NM_REQUIRE(gx <= IMG_MAX_ELEMS, "nm_conv2d_bwd: grid of %lld workgroups beyond the launch limits", (long long)gx);
            hipLaunchKernelGGL(img2d_conv_wgrad_mfma, dim3((unsigned)gx, (unsigned)s.slices), dim3(64), 0, st, g);
        } else {
            hipLaunchKernelGGL(img2d_conv_wgrad_scalar, dim3(ew_blocks(nw * s.slices)), dim3(256), 0, st, g, (long)0,
                               (long)nw);
        }
        hipLaunchKernelGGL(img2d_conv_wgrad_sum, dim3(ew_blocks(nw)), dim3(256), 0, st, g.ws, (long)s.slab, (int)s.slices,
                           (long)0, (long)nw, dfilt, accumulate_params);
    }
    if (dbias) {
        hipLaunchKernelGGL(img2d_conv_wgrad_scalar, dim3(ew_blocks(Cout * s.slices)), dim3(256), 0, st, g, (long)nw,
                           (long)s.slab);
        hipLaunchKernelGGL(img2d_conv_wgrad_sum, dim3(ew_blocks(Cout)), dim3(256), 0, st, g.ws, (long)s.slab,
                           (int)s.slices, (long)nw, (long)Cout, dbias, accumulate_params);
    }
    NM_LAUNCH_CHECK("nm_conv2d_bwd");
}

extern "C" int nm_bn2d_fwd(void* stream, const float* x, int64_t ldx, int64_t rows, int64_t C, const float* gamma,
                           const float* beta, float eps, float momentum, int training, int relu, float* moving_mean,
                           float* moving_var, float* batch_mean, float* batch_var, float* y, int64_t ldy) {
    int rc = bn_check("nm_bn2d_fwd", rows, C);
    if (rc) return rc;
    NM_REQUIRE(x && gamma && beta && y, "nm_bn2d_fwd: null pointer");
    NM_REQUIRE(ldx >= C, "nm_bn2d_fwd: ldx %lld below C %lld", (long long)ldx, (long long)C);
    NM_REQUIRE(ldy >= C, "nm_bn2d_fwd: ldy %lld below C %lld", (long long)ldy, (long long)C);
    NM_REQUIRE((double)rows * ldx < 9e18 && (double)rows * ldy < 9e18, "nm_bn2d_fwd: leading dimension too large");
    NM_REQUIRE(eps > 0.0f, "nm_bn2d_fwd: eps %g must be positive", (double)eps);
    NM_REQUIRE(momentum >= 0.0f && momentum <= 1.0f, "nm_bn2d_fwd: momentum %g outside [0, 1]", (double)momentum);
    NM_REQUIRE((moving_mean == nullptr) == (moving_var == nullptr),
               "nm_bn2d_fwd: moving_mean and moving_var come together or not at all");
    if (training)
        NM_REQUIRE(batch_mean && batch_var, "nm_bn2d_fwd: training needs batch_mean and batch_var");
    else
        NM_REQUIRE(moving_mean && moving_var, "nm_bn2d_fwd: inference needs moving_mean and moving_var");
    hipStream_t st = nm_stream(stream);
    if (training)
        hipLaunchKernelGGL(img2d_bn_stats, dim3((unsigned)((C + BN_COLS - 1) / BN_COLS)), dim3(BN_COLS, BN_LANES), 0, st, x,
                           (long)ldx, (long)rows, (int)C, momentum, moving_mean, moving_var, batch_mean, batch_var);
    hipLaunchKernelGGL(img2d_bn_apply, dim3(ew_blocks(rows * C)), dim3(256), 0, st, x, (long)ldx, (long)rows, (int)C, gamma,
                       beta, training ? batch_mean : moving_mean, training ? batch_var : moving_var, eps, relu, y,
                       (long)ldy);
    NM_LAUNCH_CHECK("nm_bn2d_fwd");
}

extern "C" int nm_bn2d_bwd(void* stream, const float* x, int64_t ldx, const float* y, int64_t ldy, const float* dy,
                           int64_t lddy, int64_t rows, int64_t C, const float* gamma, const float* batch_mean,
                           const float* batch_var, float eps, int relu, float* dx, int64_t lddx, int accumulate_dx,
                           float* dgamma, float* dbeta, int accumulate_params, float* sums) {
    int rc = bn_check("nm_bn2d_bwd", rows, C);
    if (rc) return rc;
    NM_REQUIRE(x && dy && gamma && batch_mean && batch_var && sums, "nm_bn2d_bwd: null pointer");
    NM_REQUIRE(!relu || y, "nm_bn2d_bwd: the ReLU gate needs the saved output y");
    NM_REQUIRE(ldx >= C, "nm_bn2d_bwd: ldx %lld below C %lld", (long long)ldx, (long long)C);
    NM_REQUIRE(!relu || ldy >= C, "nm_bn2d_bwd: ldy %lld below C %lld", (long long)ldy, (long long)C);
    NM_REQUIRE(lddy >= C, "nm_bn2d_bwd: lddy %lld below C %lld", (long long)lddy, (long long)C);
    NM_REQUIRE(!dx || lddx >= C, "nm_bn2d_bwd: lddx %lld below C %lld", (long long)lddx, (long long)C);
    NM_REQUIRE((double)rows * ldx < 9e18 && (double)rows * ldy < 9e18 && (double)rows * lddy < 9e18 &&
                   (double)rows * lddx < 9e18, "nm_bn2d_bwd: leading dimension too large");
    NM_REQUIRE(eps > 0.0f, "nm_bn2d_bwd: eps %g must be positive", (double)eps);
    NM_REQUIRE(!dx || (dx == dy && lddx == lddy) || !ranges_overlap(dx, lddx, rows, C, dy, lddy, rows, C),
               "nm_bn2d_bwd: dx partially overlapping dy");
    hipStream_t st = nm_stream(stream);
    hipLaunchKernelGGL(img2d_bn_bwd_sums, dim3((unsigned)((C + BN_COLS - 1) / BN_COLS)), dim3(BN_COLS, BN_LANES), 0, st, x,
                       (long)ldx, y, (long)ldy, dy, (long)lddy, (long)rows, (int)C, batch_mean, batch_var, eps, relu, sums,
                       dgamma, dbeta, accumulate_params);
    if (dx)
        hipLaunchKernelGGL(img2d_bn_bwd_dx, dim3(ew_blocks(rows * C)), dim3(256), 0, st, x, (long)ldx, y, (long)ldy, dy,
                           (long)lddy, (long)rows, (int)C, gamma, batch_mean, batch_var, eps, relu, sums, dx, (long)lddx,
                           accumulate_dx);
    NM_LAUNCH_CHECK("nm_bn2d_bwd");
}

extern "C" int nm_window2d_fwd(void* stream, const float* x, int64_t ldx, int64_t B, int64_t H, int64_t W, int64_t C,
                               int64_t kh, int64_t kw, int64_t sh, int64_t sw, int padding, int mode, float* y,
                               int64_t ldy, int32_t* argmax) {
    WindowArgs a;
    int rc = window_shape("nm_window2d_fwd", B, H, W, C, kh, kw, sh, sw, padding, mode, &a);
    if (rc) return rc;
    NM_REQUIRE(x && y, "nm_window2d_fwd: null pointer");
    NM_REQUIRE(ldx >= C, "nm_window2d_fwd: ldx %lld below C %lld", (long long)ldx, (long long)C);
    NM_REQUIRE(ldy >= C, "nm_window2d_fwd: ldy %lld below C %lld", (long long)ldy, (long long)C);
    NM_REQUIRE((double)B * H * W * ldx < 9e18 && (double)B * a.OH * a.OW * ldy < 9e18,
               "nm_window2d_fwd: leading dimension too large");
    NM_REQUIRE(!ranges_overlap(x, ldx, B * H * W, C, y, ldy, B * a.OH * a.OW, C), "nm_window2d_fwd: y overlapping x");
    hipLaunchKernelGGL(img2d_window_fwd, dim3(ew_blocks(B * a.OH * a.OW * C)), dim3(256), 0, nm_stream(stream), a, x,
                       (long)ldx, y, (long)ldy, argmax);
    NM_LAUNCH_CHECK("nm_window2d_fwd");
}

extern "C" int nm_window2d_bwd(void* stream, const float* dy, int64_t lddy, const int32_t* argmax, int64_t B, int64_t H,
                               int64_t W, int64_t C, int64_t kh, int64_t kw, int64_t sh, int64_t sw, int padding, int mode,
                               float* dx, int64_t lddx, int accumulate) {
    WindowArgs a;
    int rc = window_shape("nm_window2d_bwd", B, H, W, C, kh, kw, sh, sw, padding, mode, &a);
    if (rc) return rc;
    NM_REQUIRE(dy && dx, "nm_window2d_bwd: null pointer");
    NM_REQUIRE(mode != NM_WINDOW_MAX || argmax, "nm_window2d_bwd: the maximum's gradient needs argmax");
    NM_REQUIRE(lddy >= C, "nm_window2d_bwd: lddy %lld below C %lld", (long long)lddy, (long long)C);
    NM_REQUIRE(lddx >= C, "nm_window2d_bwd: lddx %lld below C %lld", (long long)lddx, (long long)C);
    NM_REQUIRE((double)B * H * W * lddx < 9e18 && (double)B * a.OH * a.OW * lddy < 9e18,
               "nm_window2d_bwd: leading dimension too large");
    NM_REQUIRE(!ranges_overlap(dx, lddx, B * H * W, C, dy, lddy, B * a.OH * a.OW, C), "nm_window2d_bwd: dx overlapping dy");
    hipLaunchKernelGGL(img2d_window_bwd, dim3(ew_blocks(B * H * W * C)), dim3(256), 0, nm_stream(stream), a, dy, (long)lddy,
                       argmax, dx, (long)lddx, accumulate);
    NM_LAUNCH_CHECK("nm_window2d_bwd");
}

extern "C" int nm_map_columns(void* stream, const float* src, float* dst, int64_t B, int64_t H, int64_t W, int64_t C,
                              int inverse) {
    NM_REQUIRE(B >= 1 && H >= 1 && W >= 1 && C >= 1, "nm_map_columns: bad sizes B %lld, H %lld, W %lld, C %lld", (long long)B,
               (long long)H, (long long)W, (long long)C);
    NM_REQUIRE(B <= IMG_MAX_ELEMS && H <= IMG_MAX_ELEMS && W <= IMG_MAX_ELEMS && C <= IMG_MAX_ELEMS &&
                   B * H <= IMG_MAX_ELEMS && B * H * W <= IMG_MAX_ELEMS && (double)B * H * W * C <= (double)IMG_MAX_ELEMS,
               "nm_map_columns: a map holds more than 2^31 - 1 elements");
    NM_REQUIRE(src && dst, "nm_map_columns: null pointer");
    NM_REQUIRE(!ranges_overlap(src, C, B * H * W, C, dst, C, B * H * W, C), "nm_map_columns: dst overlapping src");
    hipLaunchKernelGGL(img2d_columns, dim3(ew_blocks(B * H * W * C)), dim3(256), 0, nm_stream(stream), src, dst, (long)B,
                       (int)H, (int)W, (int)C, inverse != 0);
    NM_LAUNCH_CHECK("nm_map_columns");
}
