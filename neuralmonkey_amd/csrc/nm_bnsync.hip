// Batch norm over the rows of ALL ranks of a data-parallel job (include/nmhip_bnsync.h): what nm_bn2d_fwd / nm_bn2d_bwd
// of nm_image.hip do in one launch each, cut where the two exchanges go.  The arithmetic is that file's, expression by
// expression -- with one part the results are bit-equal to it (tests/test_bnsync_kernels_gpu.py) -- and so are the launch
// shapes: 32 channels x 32 row lanes for the column sums, one thread per element for dx.  The column-sum helper and the
// two backward kernels are restated here rather than shared: nm_image.hip and its entry points stay as they are (their
// tests count that file's kernels), and the bit-equality test is what holds the two copies together.
//
//   bnsync_part_stats   the rank's row count, rounded means and sums of squared deviations about them (two passes,
//                       summed in double, LDS partials added in lane order), written as doubles
//   bnsync_merge        one thread per channel: the parts taken in one after the other in rank order (the pairwise
//                       update of Chan, Golub and LeVeque, in double), batch statistics, moving statistics
//   bnsync_bwd_sums     the rank's two channel sums from the merged statistics
//   bnsync_bwd_dx       the input gradient from the sums of all ranks and the global row count
// No floating-point atomics anywhere.
#include "nm_common.h"
#include "../../include/nmhip_bnsync.h"

namespace {

// as in nm_image.hip: the UNBIASED batch variance enters the moving variance
constexpr bool BN_MOVING_VARIANCE_UNBIASED = true;
constexpr int BN_COLS = 32, BN_LANES = 32;
constexpr int64_t BN_MAX_ELEMS = (1ll << 31) - 1;

// the channel sums of f(row, channel) over the rows, accumulated in double, lane partials added in lane order; every
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

__global__ __launch_bounds__(BN_COLS * BN_LANES) void bnsync_part_stats(const float* __restrict__ x, long ldx, long rows,
                                                                        int C, double* __restrict__ out) {
    __shared__ double part[BN_LANES][BN_COLS + 1];
    __shared__ float smean[BN_COLS];
    const int c = blockIdx.x * BN_COLS + threadIdx.x;
    const float* xc = x + c;
    const double sum = bn_colsum(part, rows, c, C, [&](long r) { return xc[r * ldx]; });
    if (threadIdx.y == 0) smean[threadIdx.x] = (float)(sum / (double)rows);
    __syncthreads();
    const float mean = smean[threadIdx.x];                         // the rounded mean: what the deviations are taken from
    const double sq = bn_colsum(part, rows, c, C, [&](long r) { const float d = xc[r * ldx] - mean; return d * d; });
    if (threadIdx.y != 0 || c >= C) return;
    if (c == 0) out[0] = (double)rows;
    out[1 + c] = (double)mean;
    out[1 + C + c] = sq;
}

__global__ __launch_bounds__(256) void bnsync_merge(const double* __restrict__ parts, int world, int C, float momentum,
                                                    float* moving_mean, float* moving_var, float* __restrict__ batch_mean,
                                                    float* __restrict__ batch_var, double* __restrict__ total) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const long stride = 2 * (long)C + 1;
    double n = parts[0], m = parts[1 + c], m2 = parts[1 + C + c];
    for (int r = 1; r < world; ++r) {
        const double* p = parts + r * stride;
        const double nr = p[0], d = p[1 + c] - m, nn = n + nr;
        m += d * nr / nn;
        m2 += p[1 + C + c] + d * d * n * nr / nn;
        n = nn;
    }
    const long rows = (long)n;
    const float mean = (float)m;
    const float var = (float)(m2 / (double)rows);
    batch_mean[c] = mean;
    batch_var[c] = var;
    if (c == 0) total[0] = n;
    if (moving_mean) {
        const float fed = BN_MOVING_VARIANCE_UNBIASED ? var * ((float)rows / (float)(rows > 1 ? rows - 1 : 1)) : var;
        moving_mean[c] = momentum * moving_mean[c] + (1.0f - momentum) * mean;
        moving_var[c] = momentum * moving_var[c] + (1.0f - momentum) * fed;
    }
}

__global__ __launch_bounds__(BN_COLS * BN_LANES) void bnsync_bwd_sums(
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

__global__ __launch_bounds__(256) void bnsync_bwd_dx(
    const float* __restrict__ x, long ldx, const float* __restrict__ y, long ldy, const float* dy, long lddy, long rows,
    int C, const float* __restrict__ gamma, const float* __restrict__ mean, const float* __restrict__ var, float eps,
    int relu, const float* __restrict__ sums, long n, float* dx, long lddx, int accumulate) {
    const long total = rows * C;
    const float inv = 1.0f / (float)n;
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

unsigned ew_blocks(int64_t total) {
    const int64_t blocks = (total + 255) / 256;
    return (unsigned)(blocks < 1 ? 1 : (blocks > (1 << 20) ? (1 << 20) : blocks));
}

bool ranges_overlap(const float* p, int64_t ldp, const float* q, int64_t ldq, int64_t rows, int64_t cols) {
    const float* pe = p + (rows - 1) * ldp + cols;
    const float* qe = q + (rows - 1) * ldq + cols;
    return !(pe <= q || qe <= p);
}

int bn_check(const char* who, int64_t rows, int64_t C) {
    NM_REQUIRE(rows >= 1 && C >= 1, "%s: bad sizes rows %lld, C %lld", who, (long long)rows, (long long)C);
    NM_REQUIRE(rows <= BN_MAX_ELEMS && C <= BN_MAX_ELEMS && rows * C <= BN_MAX_ELEMS,
               "%s: rows * C = %lld elements beyond 2^31 - 1", who, (long long)(rows * C));
    return NM_OK;
}

}  // namespace

extern "C" int nm_bn2d_part_stats(void* stream, const float* x, int64_t ldx, int64_t rows, int64_t C, double* part) {
    int rc = bn_check("nm_bn2d_part_stats", rows, C);
    if (rc) return rc;
    NM_REQUIRE(x && part, "nm_bn2d_part_stats: null pointer");
    NM_REQUIRE(ldx >= C, "nm_bn2d_part_stats: ldx %lld below C %lld", (long long)ldx, (long long)C);
    NM_REQUIRE((double)rows * ldx < 9e18, "nm_bn2d_part_stats: leading dimension too large");
    hipLaunchKernelGGL(bnsync_part_stats, dim3((unsigned)((C + BN_COLS - 1) / BN_COLS)), dim3(BN_COLS, BN_LANES), 0,
                       nm_stream(stream), x, (long)ldx, (long)rows, (int)C, part);
    NM_LAUNCH_CHECK("nm_bn2d_part_stats");
}

extern "C" int nm_bn2d_merge(void* stream, const double* parts, int64_t world, int64_t C, float momentum,
                             float* moving_mean, float* moving_var, float* batch_mean, float* batch_var, double* total) {
    NM_REQUIRE(world >= 1 && C >= 1, "nm_bn2d_merge: bad sizes world %lld, C %lld", (long long)world, (long long)C);
    NM_REQUIRE(world <= BN_MAX_ELEMS && C <= BN_MAX_ELEMS, "nm_bn2d_merge: world %lld or C %lld beyond 2^31 - 1",
               (long long)world, (long long)C);
    NM_REQUIRE(parts && batch_mean && batch_var && total, "nm_bn2d_merge: null pointer");
    NM_REQUIRE((moving_mean == nullptr) == (moving_var == nullptr),
               "nm_bn2d_merge: moving_mean and moving_var come together or not at all");
    NM_REQUIRE(momentum >= 0.0f && momentum <= 1.0f, "nm_bn2d_merge: momentum %g outside [0, 1]", (double)momentum);
    hipLaunchKernelGGL(bnsync_merge, dim3(ew_blocks(C)), dim3(256), 0, nm_stream(stream), parts, (int)world, (int)C,
                       momentum, moving_mean, moving_var, batch_mean, batch_var, total);
    NM_LAUNCH_CHECK("nm_bn2d_merge");
}

extern "C" int nm_bn2d_bwd_sums(void* stream, const float* x, int64_t ldx, const float* y, int64_t ldy, const float* dy,
                                int64_t lddy, int64_t rows, int64_t C, const float* mean, const float* var, float eps,
                                int relu, float* sums, float* dgamma, float* dbeta, int accumulate_params) {
    int rc = bn_check("nm_bn2d_bwd_sums", rows, C);
    if (rc) return rc;
    NM_REQUIRE(x && dy && mean && var && sums, "nm_bn2d_bwd_sums: null pointer");
    NM_REQUIRE(!relu || y, "nm_bn2d_bwd_sums: the ReLU gate needs the saved output y");
    NM_REQUIRE(ldx >= C, "nm_bn2d_bwd_sums: ldx %lld below C %lld", (long long)ldx, (long long)C);
    NM_REQUIRE(!relu || ldy >= C, "nm_bn2d_bwd_sums: ldy %lld below C %lld", (long long)ldy, (long long)C);
    NM_REQUIRE(lddy >= C, "nm_bn2d_bwd_sums: lddy %lld below C %lld", (long long)lddy, (long long)C);
    NM_REQUIRE((double)rows * ldx < 9e18 && (double)rows * ldy < 9e18 && (double)rows * lddy < 9e18,
               "nm_bn2d_bwd_sums: leading dimension too large");
    NM_REQUIRE(eps > 0.0f, "nm_bn2d_bwd_sums: eps %g must be positive", (double)eps);
    hipLaunchKernelGGL(bnsync_bwd_sums, dim3((unsigned)((C + BN_COLS - 1) / BN_COLS)), dim3(BN_COLS, BN_LANES), 0,
                       nm_stream(stream), x, (long)ldx, y, (long)ldy, dy, (long)lddy, (long)rows, (int)C, mean, var, eps,
                       relu, sums, dgamma, dbeta, accumulate_params);
    NM_LAUNCH_CHECK("nm_bn2d_bwd_sums");
}

extern "C" int nm_bn2d_bwd_dx(void* stream, const float* x, int64_t ldx, const float* y, int64_t ldy, const float* dy,
                              int64_t lddy, int64_t rows, int64_t C, const float* gamma, const float* mean,
                              const float* var, float eps, int relu, const float* sums, int64_t n, float* dx,
                              int64_t lddx, int accumulate_dx) {
    int rc = bn_check("nm_bn2d_bwd_dx", rows, C);
    if (rc) return rc;
    NM_REQUIRE(x && dy && gamma && mean && var && sums && dx, "nm_bn2d_bwd_dx: null pointer");
    NM_REQUIRE(!relu || y, "nm_bn2d_bwd_dx: the ReLU gate needs the saved output y");
    NM_REQUIRE(ldx >= C, "nm_bn2d_bwd_dx: ldx %lld below C %lld", (long long)ldx, (long long)C);
    NM_REQUIRE(!relu || ldy >= C, "nm_bn2d_bwd_dx: ldy %lld below C %lld", (long long)ldy, (long long)C);
    NM_REQUIRE(lddy >= C, "nm_bn2d_bwd_dx: lddy %lld below C %lld", (long long)lddy, (long long)C);
    NM_REQUIRE(lddx >= C, "nm_bn2d_bwd_dx: lddx %lld below C %lld", (long long)lddx, (long long)C);
    NM_REQUIRE((double)rows * ldx < 9e18 && (double)rows * ldy < 9e18 && (double)rows * lddy < 9e18 &&
                   (double)rows * lddx < 9e18, "nm_bn2d_bwd_dx: leading dimension too large");
    NM_REQUIRE(eps > 0.0f, "nm_bn2d_bwd_dx: eps %g must be positive", (double)eps);
    NM_REQUIRE(n >= rows, "nm_bn2d_bwd_dx: global row count %lld below this rank's %lld", (long long)n, (long long)rows);
    NM_REQUIRE((dx == dy && lddx == lddy) || !ranges_overlap(dx, lddx, dy, lddy, rows, C),
               "nm_bn2d_bwd_dx: dx partially overlapping dy");
    hipLaunchKernelGGL(bnsync_bwd_dx, dim3(ew_blocks(rows * C)), dim3(256), 0, nm_stream(stream), x, (long)ldx, y,
                       (long)ldy, dy, (long)lddy, (long)rows, (int)C, gamma, mean, var, eps, relu, sums, (long)n, dx,
                       (long)lddx, accumulate_dx);
    NM_LAUNCH_CHECK("nm_bn2d_bwd_dx");
}
