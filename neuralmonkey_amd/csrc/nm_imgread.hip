// The image reader's device pipeline (include/nmhip_imgread.h): Pillow's convert / resize / crop and the reference's zero
// padding over a ragged chunk of decoded 8-bit images, in two launches whatever the number of images.
//
//   imgread_rows_kernel   horizontal pass, the conversion folded into the loads.  A workgroup owns ROWS_TC kept output
//                         columns x ROWS_TR source rows of one image (blockIdx.z).  The columns' bounds and their first
//                         ROWS_KCAP coefficients are staged in LDS tap-major, so the lanes of a wave -- which run along
//                         (column, channel), the contiguous axis of the scratch they write and of the pixels they read
//                         -- hit consecutive banks; taps beyond ROWS_KCAP (a downscale by more than ~15) come straight
//                         from memory, so ksize has no cap.
//   imgread_cols_kernel   vertical pass, crop, zero padding, epilogue.  A workgroup owns COLS_TR output rows x 256
//                         consecutive (column, channel) elements; a row's coefficients are one LDS address for the whole
//                         wave (a broadcast).
//
// The 8-bit targets are integer arithmetic; the F target accumulates in float64 with the product rounded before the add
// (contraction is switched off for the whole file), in tap order, as Pillow's x86 build does.  Everything read from
// device memory is clamped before it becomes an address.  No atomics.
#include "nm_common.h"
#include "../../include/nmhip_imgread.h"

// hipcc contracts a * b + c into one fused operation by default; Pillow's sums round the product first, so nothing in
// this file may be contracted.  (The sums are written with the plain operators: __dmul_rn / __dadd_rn are header
// functions compiled with contraction allowed, and fuse all the same once they are inlined.)
#pragma clang fp contract(off)

namespace {

constexpr int IMG_THREADS = 256;
constexpr int ROWS_TC = 32;      // kept output columns per workgroup of the horizontal pass
constexpr int ROWS_TR = 8;       // source rows per workgroup of the horizontal pass
constexpr int ROWS_KCAP = 64;    // taps per column staged in LDS
constexpr int COLS_TR = 4;       // output rows per workgroup of the vertical pass
constexpr int COLS_KCAP = 128;   // taps per row staged in LDS
constexpr int PRECISION_BITS = 22;

__device__ __forceinline__ long clampl(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct ImgGeom {
    int sw, sh, bands, cw, ch, row0, nrows, ksh, ksv;
    long src0, src1, scr0, scr1, hb, hk, vb, vk;
};

// image i's geometry and offsets, every field inside the limits the caller's arrays give it
__device__ __forceinline__ ImgGeom img_geom(const int64_t* __restrict__ offs, const int32_t* __restrict__ geom, long N,
                                            long i, long src_bytes, long scratch_elems, int pad_w, int pad_h) {
    const int32_t* g = geom + i * NM_IMGREAD_GEOM;
    ImgGeom o;
    o.sw = g[0] < 0 ? 0 : g[0];
    o.sh = g[1] < 0 ? 0 : g[1];
    o.bands = g[2] == 3 ? 3 : 1;
    o.cw = clampi(g[7], 0, pad_w);
    o.ch = clampi(g[8], 0, pad_h);
    o.row0 = clampi(g[9], 0, o.sh);
    o.nrows = clampi(g[10], 0, o.sh - o.row0);
    o.ksh = g[11] < 0 ? 0 : g[11];
    o.ksv = g[12] < 0 ? 0 : g[12];
    const int64_t* s = offs + 0 * (N + 1) + i;
    o.src0 = clampl(s[0], 0, src_bytes);
    o.src1 = clampl(s[1], o.src0, src_bytes);
    s = offs + 1 * (N + 1) + i;
    o.scr0 = clampl(s[0], 0, scratch_elems);
    o.scr1 = clampl(s[1], o.scr0, scratch_elems);
    o.hb = offs[2 * (N + 1) + i];
    o.hk = offs[3 * (N + 1) + i];
    o.vb = offs[4 * (N + 1) + i];
    o.vk = offs[5 * (N + 1) + i];
    return o;
}

// pair `idx` of the bounds, (0, 0) outside the array; first in [0, extent], count in [0, min(ksize, extent - first)]
__device__ __forceinline__ int2 img_bounds(const int32_t* __restrict__ bounds, long n_bounds, long idx, int extent,
                                           int ksize) {
    if (idx < 0 || idx >= n_bounds) return make_int2(0, 0);
    const int first = clampi(bounds[2 * idx], 0, extent);
    const int rest = extent - first;
    return make_int2(first, clampi(bounds[2 * idx + 1], 0, rest < ksize ? rest : ksize));
}

template <typename K>
__device__ __forceinline__ K img_coef(const K* __restrict__ coef, long n_coef, long idx) {
    return (idx < 0 || idx >= n_coef) ? (K)0 : coef[idx];
}

// one source pixel, converted: channel c of the 8-bit targets ...
__device__ __forceinline__ int img_pixel8(const uint8_t* __restrict__ p, long avail, long pix, int bands, int target,
                                          int c) {
    const long at = pix * bands;
    if (at < 0 || at + bands > avail) return 0;
    if (bands == 1) return p[at];
    if (target == NM_IMGREAD_RGB) return p[at + c];
    return (19595 * (int)p[at] + 38470 * (int)p[at + 1] + 7471 * (int)p[at + 2] + 0x8000) >> 16;
}

// ... and of F: the integer sum is exact, and the quotient taken in float64 and rounded to float32 is the correctly
// rounded float32 quotient (53 >= 2 * 24 + 2 bits: the second rounding cannot change it)
__device__ __forceinline__ float img_pixelf(const uint8_t* __restrict__ p, long avail, long pix, int bands) {
    const long at = pix * bands;
    if (at < 0 || at + bands > avail) return 0.0f;
    if (bands == 1) return (float)p[at];
    const int sum = 299 * (int)p[at] + 587 * (int)p[at + 1] + 114 * (int)p[at + 2];
    return (float)((double)sum / 1000.0);
}

__device__ __forceinline__ uint8_t img_clip8(int acc) {
    const int v = acc >> PRECISION_BITS;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// T: the pass type (uint8_t for L and RGB, float for F); K: its coefficients (int32_t, double)
template <typename T, typename K>
__global__ __launch_bounds__(IMG_THREADS) void imgread_rows_kernel(
    const uint8_t* __restrict__ src, long src_bytes, const int64_t* __restrict__ offs, const int32_t* __restrict__ geom,
    long N, const int32_t* __restrict__ bounds, long n_bounds, const K* __restrict__ coef, long n_coef, int target,
    int pad_w, T* __restrict__ scratch, long scratch_elems) {
    __shared__ K k_lds[ROWS_KCAP * ROWS_TC];                       // [tap][column]
    __shared__ int2 b_lds[ROWS_TC];
    const long i = blockIdx.z;
    const ImgGeom g = img_geom(offs, geom, N, i, src_bytes, scratch_elems, pad_w, 1 << 30);
    const int x0 = blockIdx.x * ROWS_TC, r0 = blockIdx.y * ROWS_TR;
    if (x0 >= g.cw || r0 >= g.nrows) return;                       // (block-uniform)
    const int C = target == NM_IMGREAD_RGB ? 3 : 1;
    const int ncols = g.cw - x0 < ROWS_TC ? g.cw - x0 : ROWS_TC;
    const int nrows = g.nrows - r0 < ROWS_TR ? g.nrows - r0 : ROWS_TR;
    const int staged = g.ksh < ROWS_KCAP ? g.ksh : ROWS_KCAP;

    for (int col = threadIdx.x; col < ncols; col += IMG_THREADS)
        b_lds[col] = img_bounds(bounds, n_bounds, g.hb + x0 + col, g.sw, g.ksh);
    for (int e = threadIdx.x; e < ncols * staged; e += IMG_THREADS) {
        const int col = e / staged, t = e - col * staged;          // consecutive threads read consecutive coefficients
        k_lds[t * ROWS_TC + col] = img_coef(coef, n_coef, g.hk + (long)(x0 + col) * g.ksh + t);
    }
    __syncthreads();

    const uint8_t* p = src + g.src0;
    const long avail = g.src1 - g.src0;
    const int per_row = ncols * C;
    for (int e = threadIdx.x; e < nrows * per_row; e += IMG_THREADS) {
        const int r = e / per_row, rest = e - r * per_row;
        const int col = rest / C, c = rest - col * C;
        const int2 b = b_lds[col];
        const long row_pix = (long)(g.row0 + r0 + r) * g.sw + b.x;
        const long tail_at = g.hk + (long)(x0 + col) * g.ksh;      // the column's coefficients in memory
        T value;
        if constexpr (sizeof(T) == 1) {
            int acc = 1 << (PRECISION_BITS - 1);
            for (int t = 0; t < b.y; ++t) {
                const int k = t < staged ? (int)k_lds[t * ROWS_TC + col] : (int)img_coef(coef, n_coef, tail_at + t);
                acc += img_pixel8(p, avail, row_pix + t, g.bands, target, c) * k;
            }
            value = img_clip8(acc);
        } else {
            double acc = 0.0;
            for (int t = 0; t < b.y; ++t) {
                const double k = t < staged ? (double)k_lds[t * ROWS_TC + col] : (double)img_coef(coef, n_coef, tail_at + t);
                acc = acc + (double)img_pixelf(p, avail, row_pix + t, g.bands) * k;       // (uncontracted: see above)
            }
            value = (float)acc;
        }
        const long at = g.scr0 + ((long)(r0 + r) * g.cw + x0 + col) * C + c;
        if (at < g.scr1) scratch[at] = value;
    }
}

template <typename T, typename K>
__global__ __launch_bounds__(IMG_THREADS) void imgread_cols_kernel(
    const T* __restrict__ scratch, long scratch_elems, const int64_t* __restrict__ offs, const int32_t* __restrict__ geom,
    long N, const int32_t* __restrict__ bounds, long n_bounds, const K* __restrict__ coef, long n_coef, int target,
    int pad_w, int pad_h, const double* __restrict__ sub, double divide, int epilogue, float* __restrict__ out, long ld) {
    __shared__ K k_lds[COLS_TR * COLS_KCAP];                       // [row][tap]
    __shared__ int2 b_lds[COLS_TR];
    const long i = blockIdx.z;
    const ImgGeom g = img_geom(offs, geom, N, i, 0, scratch_elems, pad_w, pad_h);
    const int C = target == NM_IMGREAD_RGB ? 3 : 1;
    const int y0 = blockIdx.y * COLS_TR;
    const int nrows = pad_h - y0 < COLS_TR ? pad_h - y0 : COLS_TR;
    const int staged = g.ksv < COLS_KCAP ? g.ksv : COLS_KCAP;

    if (threadIdx.x < COLS_TR) {
        const int y = y0 + threadIdx.x;
        int2 b = make_int2(0, 0);
        if (y < g.ch) {
            b = img_bounds(bounds, n_bounds, g.vb + y, g.row0 + g.nrows, g.ksv);
            // the scratch holds the source rows row0 .. row0 + nrows only
            if (b.x < g.row0) b = make_int2(0, 0);
        }
        b_lds[threadIdx.x] = b;
    }
    for (int e = threadIdx.x; e < COLS_TR * staged; e += IMG_THREADS) {
        const int r = e / staged, t = e - r * staged;
        k_lds[r * COLS_KCAP + t] = (y0 + r < g.ch) ? img_coef(coef, n_coef, g.vk + (long)(y0 + r) * g.ksv + t) : (K)0;
    }
    __syncthreads();

    const int e = blockIdx.x * IMG_THREADS + threadIdx.x;          // (column, channel) of the padded row
    if (e >= pad_w * C) return;
    const int x = e / C, c = e - x * C;
    const long row_elems = (long)g.cw * C;
    const double mean = (epilogue && sub != nullptr) ? sub[c] : 0.0;
    for (int r = 0; r < nrows; ++r) {
        const int2 b = b_lds[r];
        float value = 0.0f;
        if (x < g.cw && b.y > 0) {
            const long first = g.scr0 + (long)(b.x - g.row0) * row_elems + e;
            const long tail_at = g.vk + (long)(y0 + r) * g.ksv;
            if constexpr (sizeof(T) == 1) {
                int acc = 1 << (PRECISION_BITS - 1);
                for (int t = 0; t < b.y; ++t) {
                    const int k = t < staged ? (int)k_lds[r * COLS_KCAP + t] : (int)img_coef(coef, n_coef, tail_at + t);
                    const long at = first + t * row_elems;
                    acc += (at < g.scr1 ? (int)scratch[at] : 0) * k;
                }
                value = (float)img_clip8(acc);
            } else {
                double acc = 0.0;
                for (int t = 0; t < b.y; ++t) {
                    const double k =
                        t < staged ? (double)k_lds[r * COLS_KCAP + t] : (double)img_coef(coef, n_coef, tail_at + t);
                    const long at = first + t * row_elems;
                    acc = acc + (double)(at < g.scr1 ? scratch[at] : 0.0f) * k;        // (uncontracted: see above)
                }
                value = (float)acc;
            }
        }
        if (epilogue) value = (float)(((double)value - mean) / divide);
        out[(i * pad_h + y0 + r) * ld + e] = value;
    }
}

bool img_target_ok(int target) { return target == NM_IMGREAD_L || target == NM_IMGREAD_RGB || target == NM_IMGREAD_F; }

}  // namespace

extern "C" {

int nm_imgread_rows(void* stream, const void* src, int64_t src_bytes, const int64_t* offs, const int32_t* geom, int64_t N,
                    const int32_t* bounds, int64_t n_bounds, const void* coef, int64_t n_coef, int target, int64_t pad_w,
                    int64_t max_rows, void* scratch, int64_t scratch_elems) {
    NM_REQUIRE(N >= 1 && N <= NM_IMGREAD_MAX_IMAGES, "nm_imgread_rows: N = %lld images outside 1..%d", (long long)N,
               NM_IMGREAD_MAX_IMAGES);
    NM_REQUIRE(img_target_ok(target), "nm_imgread_rows: unknown target %d (0 L, 1 RGB, 2 F)", target);
    NM_REQUIRE(pad_w >= 1 && pad_w <= (1ll << 31) - 1, "nm_imgread_rows: pad_w %lld outside 1 .. 2^31 - 1",
               (long long)pad_w);
    NM_REQUIRE(max_rows >= 0 && max_rows <= (1ll << 31) - 1, "nm_imgread_rows: max_rows %lld outside 0 .. 2^31 - 1",
               (long long)max_rows);
    NM_REQUIRE(src_bytes >= 0 && scratch_elems >= 0 && n_bounds >= 0 && n_coef >= 0,
               "nm_imgread_rows: negative size (src_bytes %lld, scratch_elems %lld, n_bounds %lld, n_coef %lld)",
               (long long)src_bytes, (long long)scratch_elems, (long long)n_bounds, (long long)n_coef);
    if (max_rows == 0 || src_bytes == 0) return NM_OK;
    NM_REQUIRE(src != nullptr && offs != nullptr && geom != nullptr && bounds != nullptr && coef != nullptr &&
                   scratch != nullptr,
               "nm_imgread_rows: null pointer (src, offs, geom, bounds, coef or scratch)");
    const int64_t gx = (pad_w + ROWS_TC - 1) / ROWS_TC, gy = (max_rows + ROWS_TR - 1) / ROWS_TR;
    NM_REQUIRE(gy <= NM_MAX_GRID_Y, "nm_imgread_rows: max_rows %lld beyond one grid", (long long)max_rows);
    const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)N);
    if (target == NM_IMGREAD_F)
        hipLaunchKernelGGL((imgread_rows_kernel<float, double>), grid, dim3(IMG_THREADS), 0, nm_stream(stream),
                           static_cast<const uint8_t*>(src), (long)src_bytes, offs, geom, (long)N, bounds, (long)n_bounds,
                           static_cast<const double*>(coef), (long)n_coef, target, (int)pad_w,
                           static_cast<float*>(scratch), (long)scratch_elems);
    else
        hipLaunchKernelGGL((imgread_rows_kernel<uint8_t, int32_t>), grid, dim3(IMG_THREADS), 0, nm_stream(stream),
                           static_cast<const uint8_t*>(src), (long)src_bytes, offs, geom, (long)N, bounds, (long)n_bounds,
                           static_cast<const int32_t*>(coef), (long)n_coef, target, (int)pad_w,
                           static_cast<uint8_t*>(scratch), (long)scratch_elems);
    NM_LAUNCH_CHECK("nm_imgread_rows");
}

int nm_imgread_cols(void* stream, const void* scratch, int64_t scratch_elems, const int64_t* offs, const int32_t* geom,
                    int64_t N, const int32_t* bounds, int64_t n_bounds, const void* coef, int64_t n_coef, int target,
                    int64_t pad_w, int64_t pad_h, const double* sub, double divide, float* out, int64_t ld) {
    NM_REQUIRE(N >= 1 && N <= NM_IMGREAD_MAX_IMAGES, "nm_imgread_cols: N = %lld images outside 1..%d", (long long)N,
               NM_IMGREAD_MAX_IMAGES);
    NM_REQUIRE(img_target_ok(target), "nm_imgread_cols: unknown target %d (0 L, 1 RGB, 2 F)", target);
    NM_REQUIRE(pad_w >= 1 && pad_h >= 1 && pad_w <= (1ll << 31) - 1 && pad_h <= (1ll << 31) - 1,
               "nm_imgread_cols: pad_w %lld, pad_h %lld outside 1 .. 2^31 - 1", (long long)pad_w, (long long)pad_h);
    const int64_t C = target == NM_IMGREAD_RGB ? 3 : 1;
    NM_REQUIRE(pad_w * C <= (1ll << 31) - 1 && ld >= pad_w * C, "nm_imgread_cols: ld %lld below pad_w * C = %lld",
               (long long)ld, (long long)(pad_w * C));
    NM_REQUIRE(ld <= ((1ll << 31) - 1) / pad_h && pad_h * ld <= ((1ll << 31) - 1) / N,
               "nm_imgread_cols: N * pad_h * ld = %lld * %lld * %lld elements beyond 2^31 - 1", (long long)N,
               (long long)pad_h, (long long)ld);
    NM_REQUIRE(divide != 0.0 && divide == divide, "nm_imgread_cols: divide %g", divide);
    NM_REQUIRE(scratch_elems >= 0 && n_bounds >= 0 && n_coef >= 0,
               "nm_imgread_cols: negative size (scratch_elems %lld, n_bounds %lld, n_coef %lld)",
               (long long)scratch_elems, (long long)n_bounds, (long long)n_coef);
    NM_REQUIRE(scratch != nullptr && offs != nullptr && geom != nullptr && bounds != nullptr && coef != nullptr &&
                   out != nullptr,
               "nm_imgread_cols: null pointer (scratch, offs, geom, bounds, coef or out)");
    const int64_t gx = (pad_w * C + IMG_THREADS - 1) / IMG_THREADS, gy = (pad_h + COLS_TR - 1) / COLS_TR;
    NM_REQUIRE(gy <= NM_MAX_GRID_Y, "nm_imgread_cols: pad_h %lld beyond one grid", (long long)pad_h);
    const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)N);
    const int epilogue = (sub != nullptr || divide != 1.0) ? 1 : 0;
    if (target == NM_IMGREAD_F)
        hipLaunchKernelGGL((imgread_cols_kernel<float, double>), grid, dim3(IMG_THREADS), 0, nm_stream(stream),
                           static_cast<const float*>(scratch), (long)scratch_elems, offs, geom, (long)N, bounds,
                           (long)n_bounds, static_cast<const double*>(coef), (long)n_coef, target, (int)pad_w, (int)pad_h,
                           sub, divide, epilogue, out, (long)ld);
    else
        hipLaunchKernelGGL((imgread_cols_kernel<uint8_t, int32_t>), grid, dim3(IMG_THREADS), 0, nm_stream(stream),
                           static_cast<const uint8_t*>(scratch), (long)scratch_elems, offs, geom, (long)N, bounds,
                           (long)n_bounds, static_cast<const int32_t*>(coef), (long)n_coef, target, (int)pad_w,
                           (int)pad_h, sub, divide, epilogue, out, (long)ld);
    NM_LAUNCH_CHECK("nm_imgread_cols");
}

int nm_imgread_check(const int64_t* host_offs, const int32_t* host_geom, int64_t N, int target, int64_t pad_w,
                     int64_t pad_h) {
    NM_REQUIRE(host_offs != nullptr && host_geom != nullptr, "nm_imgread_check: null pointer (host_offs or host_geom)");
    NM_REQUIRE(N >= 1 && N <= NM_IMGREAD_MAX_IMAGES, "nm_imgread_check: N = %lld images outside 1..%d", (long long)N,
               NM_IMGREAD_MAX_IMAGES);
    NM_REQUIRE(img_target_ok(target), "nm_imgread_check: unknown target %d (0 L, 1 RGB, 2 F)", target);
    NM_REQUIRE(pad_w >= 1 && pad_h >= 1, "nm_imgread_check: pad_w %lld, pad_h %lld below 1", (long long)pad_w,
               (long long)pad_h);
    const int64_t C = target == NM_IMGREAD_RGB ? 3 : 1;
    for (int64_t i = 0; i < N; ++i) {
        const int32_t* g = host_geom + i * NM_IMGREAD_GEOM;
        NM_REQUIRE(g[2] == 1 || g[2] == 3, "nm_imgread_check: image %lld has %d bands (1 or 3)", (long long)i, g[2]);
        for (int f = 0; f < 13; ++f)
            NM_REQUIRE(g[f] >= 0, "nm_imgread_check: image %lld has a negative geometry field %d", (long long)i, f);
        NM_REQUIRE(g[7] <= pad_w && g[8] <= pad_h, "nm_imgread_check: image %lld copies %d x %d into %lld x %lld",
                   (long long)i, g[7], g[8], (long long)pad_w, (long long)pad_h);
        NM_REQUIRE((int64_t)g[9] + g[10] <= g[1], "nm_imgread_check: image %lld reads rows %d + %d of %d", (long long)i,
                   g[9], g[10], g[1]);
        const int64_t need[NM_IMGREAD_OFFS] = {(int64_t)g[0] * g[1] * g[2], (int64_t)g[10] * g[7] * C, g[7],
                                               (int64_t)g[7] * g[11], g[8], (int64_t)g[8] * g[12]};
        for (int f = 0; f < NM_IMGREAD_OFFS; ++f) {
            const int64_t a = host_offs[f * (N + 1) + i], b = host_offs[f * (N + 1) + i + 1];
            NM_REQUIRE(a >= 0 && b >= a && b - a >= need[f],
                       "nm_imgread_check: image %lld needs %lld entries of array %d, its offsets give %lld .. %lld",
                       (long long)i, (long long)need[f], f, (long long)a, (long long)b);
        }
    }
    return NM_OK;
}

}  // extern "C"
