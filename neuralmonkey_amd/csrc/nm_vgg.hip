// The frozen ImageNet networks (include/nmhip_vgg.h): the device work of encoders/imagenet_encoder.py -- TF-slim's VGG is
// a chain of slim.conv2d layers, each a stride-1 convolution + bias + ReLU, forward only.  Maps are NHWC with a leading
// dimension, filters TensorFlow's [k, k, Cin, Cout].
//
//   vgg_conv_act_mfma   implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32).  M runs over the FLATTENED output positions
//                       p = (b*OH + oy)*OW + ox, N over the output channels, K over the flattened filter index
//                       kk = (ky*k + kx)*Cin + ci -- the filter IS the row-major [K, Cout] matrix of that product.  A
//                       workgroup of 4 waves owns BM positions x BN channels; per chunk of 16 values of kk it gathers the
//                       A tile (every position finds its own input pixel for the chunk's taps, zero outside the map, so a
//                       tile may span rows and images) and the B tile into LDS, one chunk ahead in registers while the
//                       matrix cores work on the chunk in LDS.  img2d_conv_mfma of nm_image.hip tiles ONE output row
//                       (128 positions of it) and stages 16 input channels of one filter row at a time: at VGG's 56-, 28-
//                       and 14-wide maps its tiles are 44 %, 22 % and 11 % full, and at Cin = 3 its chunks 3/16 full.
//                       Here a tile is full whenever B*OH*OW >= BM and the first layer is one K of 27 (two chunks).
//                       Bias and ReLU are applied to the accumulators.  The sum over kk runs in one fixed order.
// No floating-point atomics anywhere.
#include "nm_common.h"
#include "../../include/nmhip_image.h"
#include "../../include/nmhip_vgg.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int VGG_CH = 16;           // values of the flattened filter index staged at a time
constexpr int VGG_MAX_K = 7;         // widest filter (fc6 of VGG, were it run here)
constexpr int VGG_OUTSIDE = -(1 << 20);   // the row of a position past the last one: every tap of it lies outside the map

struct ActArgs {
    const float* x;          // [B, IH, IW, Cin] rows of ldx
    long ldx;
    const float* W;          // [k*k*Cin, Cout]
    const float* bias;       // [Cout] or null
    float* y;                // [P, Cout] rows of ldy
    long ldy;
    long P;                  // B*OH*OW
    int IH, IW, Cin, OH, OW, Cout, k, pt, pl, K, relu;
};

// VEC: Cin, Cout and ldx are multiples of 4 and x, W are 16-byte aligned -- four consecutive kk share a tap and are four
// adjacent channels of one pixel, so both tiles are gathered with 16-byte loads.
template <int BM, int BN, int WM, int WN, bool VEC>
__global__ __launch_bounds__(256) void vgg_conv_act_mfma(ActArgs a) {
    static_assert(WM * WN == 4 && BM % (32 * WM) == 0 && BN % (32 * WN) == 0 && BM % 64 == 0 && BN % 64 == 0, "tile");
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;            // 32 x 32 accumulators of a wave
    constexpr int LDA = BM + 2, LDB = BN + 4;                      // rows apart in banks for the staging writes
    constexpr int NA = VEC ? BM / 64 : BM / 16, NB = VEC ? BN / 64 : BN / 16;      // staged values per thread
    __shared__ float As[VGG_CH][LDA];                              // [kk of the chunk][position]
    __shared__ __attribute__((aligned(16))) float Bs[VGG_CH][LDB]; // [kk of the chunk][output channel]
    __shared__ int Prow[BM], Pcol[BM], Pimg[BM];                   // oy - pt, ox - pl and b*IH of the tile's positions

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, half = lane >> 5;
    const long p0 = (long)blockIdx.x * BM;
    const int c0 = blockIdx.y * BN;
    const int k = a.k;

    for (int i = tid; i < BM; i += 256) {
        const long p = p0 + i;
        int row = VGG_OUTSIDE, col = 0, img = 0;
        if (p < a.P) {
            const long q = p / a.OW;
            col = (int)(p - q * a.OW) - a.pl;
            const long b = q / a.OH;
            row = (int)(q - b * a.OH) - a.pt;
            img = (int)(b * a.IH);
        }
        Prow[i] = row; Pcol[i] = col; Pimg[i] = img;
    }
    __syncthreads();

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    float4 ra4[VEC ? NA : 1], rb4[VEC ? NB : 1];
    float ra1[VEC ? 1 : NA], rb1[VEC ? 1 : NB];

    // the chunk's values from global memory into registers
    auto fetch = [&](int chunk) {
        const int kk0 = chunk * VGG_CH;
        if constexpr (VEC) {
            const int kk = kk0 + 4 * (tid & 3);                    // this thread's four kk: one tap, channels ci .. ci + 3
            const int tap = kk / a.Cin, ci = kk - tap * a.Cin, ky = tap / k, kx = tap - ky * k;
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int q = (tid >> 2) + 64 * i;
                const int iy = Prow[q] + ky, ix = Pcol[q] + kx;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (kk < a.K && iy >= 0 && iy < a.IH && ix >= 0 && ix < a.IW)
                    v = *reinterpret_cast<const float4*>(a.x + ((long)(Pimg[q] + iy) * a.IW + ix) * a.ldx + ci);
                ra4[i] = v;
            }
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int idx = tid + 256 * i, r = idx / (BN / 4), c = 4 * (idx % (BN / 4));
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (kk0 + r < a.K && c0 + c < a.Cout)
                    v = *reinterpret_cast<const float4*>(a.W + (long)(kk0 + r) * a.Cout + c0 + c);
                rb4[i] = v;
            }
        } else {
            const int kk = kk0 + (tid & 15);
            const int tap = kk / a.Cin, ci = kk - tap * a.Cin, ky = tap / k, kx = tap - ky * k;
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int q = (tid >> 4) + 16 * i;
                const int iy = Prow[q] + ky, ix = Pcol[q] + kx;
                float v = 0.0f;
                if (kk < a.K && iy >= 0 && iy < a.IH && ix >= 0 && ix < a.IW)
                    v = a.x[((long)(Pimg[q] + iy) * a.IW + ix) * a.ldx + ci];
                ra1[i] = v;
            }
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int idx = tid + 256 * i, r = idx / BN, c = idx % BN;
                float v = 0.0f;
                if (kk0 + r < a.K && c0 + c < a.Cout) v = a.W[(long)(kk0 + r) * a.Cout + c0 + c];
                rb1[i] = v;
            }
        }
    };
    // ... and from the registers into LDS
    auto stage = [&]() {
        if constexpr (VEC) {
            const int g = 4 * (tid & 3);
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int q = (tid >> 2) + 64 * i;
                As[g + 0][q] = ra4[i].x; As[g + 1][q] = ra4[i].y; As[g + 2][q] = ra4[i].z; As[g + 3][q] = ra4[i].w;
            }
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int idx = tid + 256 * i, r = idx / (BN / 4), c = 4 * (idx % (BN / 4));
                *reinterpret_cast<float4*>(&Bs[r][c]) = rb4[i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < NA; ++i) As[tid & 15][(tid >> 4) + 16 * i] = ra1[i];
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int idx = tid + 256 * i;
                Bs[idx / BN][idx % BN] = rb1[i];
            }
        }
    };

    const int m0 = (wave / WN) * (TM * 32), n0 = (wave % WN) * (TN * 32);
    const int chunks = (a.K + VGG_CH - 1) / VGG_CH;
    fetch(0);
    for (int chunk = 0; chunk < chunks; ++chunk) {
        stage();
        __syncthreads();
        if (chunk + 1 < chunks) fetch(chunk + 1);                  // in flight under the matrix cores
#pragma unroll
        for (int kk = 0; kk < VGG_CH; kk += 2) {
            float av[TM], bv[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) av[i] = As[kk + half][m0 + 32 * i + l32];
#pragma unroll
            for (int j = 0; j < TN; ++j) bv[j] = Bs[kk + half][n0 + 32 * j + l32];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }

    // C/D layout of v_mfma_f32_32x32x2_f32: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int co = c0 + n0 + 32 * j + l32;
        if (co >= a.Cout) continue;
        const float bias = a.bias ? a.bias[co] : 0.0f;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long p = p0 + m0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (p >= a.P) continue;
                float v = acc[i][j][r] + bias;
                if (a.relu) v = fmaxf(v, 0.0f);
                a.y[p * a.ldy + co] = v;
            }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
constexpr int64_t VGG_MAX_ELEMS = (1ll << 31) - 1;

bool vgg_ranges_overlap(const float* p, int64_t ldp, int64_t prows, int64_t pcols, const float* q, int64_t ldq,
                        int64_t qrows, int64_t qcols) {
    const float* pe = p + (prows - 1) * ldp + pcols;
    const float* qe = q + (qrows - 1) * ldq + qcols;
    return !(pe <= q || qe <= p);
}

template <int BM, int BN, int WM, int WN>
int vgg_launch(hipStream_t st, const ActArgs& a, bool vec) {
    const int64_t gx = (a.P + BM - 1) / BM, gy = (a.Cout + BN - 1) / BN;
    NM_REQUIRE(gx <= VGG_MAX_ELEMS && gy <= NM_MAX_GRID_Y,
               "nm_conv2d_act_fwd: grid of %lld x %lld workgroups beyond the launch limits", (long long)gx, (long long)gy);
    if (vec)
        hipLaunchKernelGGL((vgg_conv_act_mfma<BM, BN, WM, WN, true>), dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((vgg_conv_act_mfma<BM, BN, WM, WN, false>), dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st, a);
    NM_LAUNCH_CHECK("nm_conv2d_act_fwd");
}

// algo 0, from tools/bench_vgg.py's times of the tiles on VGG-16's layer shapes at B = 5 and B = 32 (DESIGN.md section
// 4.20): 128 x 64 where it gives every compute unit (256) two workgroups, 64 x 64 below that.  (A 128 x 128 tile was
// measured too and dropped: never more than 4 % ahead of 128 x 64, up to 9 % behind it.)
int vgg_auto_tile(int64_t P, int64_t Cout) { return ((P + 127) / 128) * ((Cout + 63) / 64) >= 512 ? 1 : 2; }

}  // namespace

extern "C" int nm_conv2d_act_fwd(void* stream, const float* x, int64_t ldx, int64_t B, int64_t H, int64_t W, int64_t Cin,
                                 const float* filt, int64_t k, int64_t Cout, int padding, const float* bias, int relu,
                                 float* y, int64_t ldy, int algo) {
    const char* who = "nm_conv2d_act_fwd";
    NM_REQUIRE(B >= 1 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1 && k >= 1,
               "%s: bad sizes B %lld, H %lld, W %lld, Cin %lld, Cout %lld, k %lld", who, (long long)B, (long long)H,
               (long long)W, (long long)Cin, (long long)Cout, (long long)k);
    NM_REQUIRE(k <= VGG_MAX_K, "%s: the kernel takes k <= %d, not %lld", who, VGG_MAX_K, (long long)k);
    NM_REQUIRE(padding == NM_PAD_VALID || padding == NM_PAD_SAME, "%s: padding %d (0 VALID, 1 SAME)", who, padding);
    NM_REQUIRE(padding == NM_PAD_SAME || (H >= k && W >= k),
               "%s: VALID padding with a %lld x %lld map below the %lld x %lld filter", who, (long long)H, (long long)W,
               (long long)k, (long long)k);
    const int64_t mx = Cin > Cout ? Cin : Cout;
    NM_REQUIRE(B <= VGG_MAX_ELEMS && H <= VGG_MAX_ELEMS && W <= VGG_MAX_ELEMS && Cin <= VGG_MAX_ELEMS &&
                   Cout <= VGG_MAX_ELEMS && B * H <= VGG_MAX_ELEMS && B * H * W <= VGG_MAX_ELEMS &&
                   (double)B * H * W * mx <= (double)VGG_MAX_ELEMS && (double)k * k * Cin * Cout <= (double)VGG_MAX_ELEMS,
               "%s: a map or the filter holds more than 2^31 - 1 elements", who);
    NM_REQUIRE(x && filt && y, "%s: null pointer", who);
    NM_REQUIRE(ldx >= Cin, "%s: ldx %lld below Cin %lld", who, (long long)ldx, (long long)Cin);
    NM_REQUIRE(ldy >= Cout, "%s: ldy %lld below Cout %lld", who, (long long)ldy, (long long)Cout);
    const int64_t OH = padding == NM_PAD_SAME ? H : H - k + 1, OW = padding == NM_PAD_SAME ? W : W - k + 1;
    const int64_t P = B * OH * OW;
    NM_REQUIRE((double)B * H * W * ldx < 9e18 && (double)P * ldy < 9e18, "%s: leading dimension too large", who);
    NM_REQUIRE(!vgg_ranges_overlap(x, ldx, B * H * W, Cin, y, ldy, P, Cout), "%s: y overlapping x", who);
    NM_REQUIRE(algo >= 0 && algo <= 2, "%s: algo %d (0 auto, 1 128x64, 2 64x64)", who, algo);
    ActArgs a;
    a.x = x; a.ldx = ldx; a.W = filt; a.bias = bias; a.y = y; a.ldy = ldy; a.P = P;
    a.IH = (int)H; a.IW = (int)W; a.Cin = (int)Cin; a.OH = (int)OH; a.OW = (int)OW; a.Cout = (int)Cout; a.k = (int)k;
    a.pt = a.pl = padding == NM_PAD_SAME ? (int)((k - 1) / 2) : 0;
    a.K = (int)(k * k * Cin); a.relu = relu != 0;
    const bool vec = Cin % 4 == 0 && Cout % 4 == 0 && ldx % 4 == 0 && nm_aligned16(x) && nm_aligned16(filt);
    hipStream_t st = nm_stream(stream);
    switch (algo ? algo : vgg_auto_tile(P, Cout)) {
        case 1: return vgg_launch<128, 64, 2, 2>(st, a, vec);
        default: return vgg_launch<64, 64, 2, 2>(st, a, vec);
    }
}
