// The speech front end (include/nmhip_speech.h): the published algorithm of python_speech_features 0.6 -- what the
// reference's processors/speech.py delegates mfcc / fbank / logfbank / ssc / delta to -- over a ragged batch of
// utterances, in fp32.
//
//   speech_frames_kernel   one workgroup (4 waves) per frame.  The frame's samples are pre-emphasised and windowed on the
//                          way into LDS, at their bit-reversed places; a radix-2 FFT runs there in log2(nfft) passes of
//                          nfft/2 butterflies (complex fp32 as float2: 8-byte LDS accesses; 4096 points are 32 KB), its
//                          twiddles read from the host's table.  Then the power spectrum of the bins 0..nfft/2, the
//                          frame's energy (lane sums, 64-wide shuffle reduction, the four waves' sums added in a fixed
//                          order), the mel filters -- a wavefront per filter, lanes striding over the filter's own bin
//                          range -- eps, log, the numcep x nfilt DCT-and-lifter product and one coalesced row store.
//   speech_deltas_kernel   one order of deltas from column block o to block o + 1, a thread per (row, column), the row
//                          clamped to its own utterance.
//
// Offsets are device data and are never trusted with an address: see the header.  No atomics anywhere.
#include "nm_common.h"
#include "../../include/nmhip_speech.h"

namespace {

constexpr int SPEECH_THREADS = 256;
constexpr float SPEECH_EPS = 2.220446049250313e-16f;               // 2^-52, exact in fp32
constexpr float SPEECH_LOG_EPS = (float)-36.043653389117154;       // log(2^-52), rounded once

// the utterance that owns output row r: the last u in [0, U) with off[u] <= r (U - 1 or 0 if the offsets are not sorted)
__device__ __forceinline__ long speech_owner(const int64_t* __restrict__ off, long U, long r) {
    long lo = 0, hi = U - 1;
    while (lo < hi) {
        const long mid = (lo + hi + 1) >> 1;
        if (off[mid] <= r) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ float speech_log(float v) { return v == 0.0f ? SPEECH_LOG_EPS : logf(v); }

__global__ __launch_bounds__(SPEECH_THREADS) void speech_frames_kernel(
    const float* __restrict__ wav, const int64_t* __restrict__ sample_off, const int64_t* __restrict__ frame_off, long U,
    long total_samples, long total_frames, long fl, long fs, int nfft, int log2n, float preemph,
    const float* __restrict__ window, const float2* __restrict__ twiddles, const float* __restrict__ fb,
    const int32_t* __restrict__ fb_range, int nfilt, const float* __restrict__ dct, int numcep,
    const float* __restrict__ R, int mode, int append_energy, float* __restrict__ out, long ld) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int nbins = nfft / 2 + 1;
    float2* a = reinterpret_cast<float2*>(smem);                                        // [nfft]
    float* P = reinterpret_cast<float*>(smem + (size_t)nfft * sizeof(float2));          // [nbins], padded to 4
    float* F = P + ((nbins + 3) & ~3);                                                  // [nfilt], padded to 4
    float* G = F + ((nfilt + 3) & ~3);                                                  // [nfilt]: ssc's numerators
    float* red = G + ((nfilt + 3) & ~3);                                                // [4]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long row = blockIdx.x;
    const int width = mode == NM_SPEECH_MFCC ? numcep : nfilt;
    float* orow = out + row * ld;

    const long u = speech_owner(frame_off, U, row);
    const long f0 = frame_off[u], f1 = frame_off[u + 1];
    if (row < f0 || row >= f1) {                                   // (wave- and block-uniform) nobody's row
        for (int c = tid; c < width; c += SPEECH_THREADS) orow[c] = 0.0f;
        return;
    }
    long s0 = sample_off[u], s1 = sample_off[u + 1];
    s0 = s0 < 0 ? 0 : (s0 > total_samples ? total_samples : s0);
    s1 = s1 < s0 ? s0 : (s1 > total_samples ? total_samples : s1);
    const long first = s0 + (row - f0) * fs;                       // the frame's first sample
    const int taken = (int)(fl < nfft ? fl : nfft);                // a frame longer than the transform is truncated

    // ---- samples into LDS, bit-reversed: y[g] = x[g] - preemph * x[g-1], x[s0] itself at the utterance's start ----
    for (int i = tid; i < nfft; i += SPEECH_THREADS) {
        float y = 0.0f;
        const long g = first + i;
        if (i < taken && g >= s0 && g < s1) {
            const float x = wav[g];
            y = g == s0 ? x : x - preemph * wav[g - 1];
            y *= window[i];
        }
        a[__brev((unsigned)i) >> (32 - log2n)] = make_float2(y, 0.0f);
    }
    __syncthreads();

    // ---- radix-2 decimation in time ----
    for (int s = 1; s <= log2n; ++s) {
        const int m = 1 << (s - 1);
        for (int b = tid; b < nfft / 2; b += SPEECH_THREADS) {
            const int j = b & (m - 1);
            const int lo = ((b >> (s - 1)) << s) + j;
            const float2 w = twiddles[j << (log2n - s)];
            const float2 p = a[lo], q = a[lo + m];
            const float2 v = make_float2(q.x * w.x - q.y * w.y, q.x * w.y + q.y * w.x);
            a[lo] = make_float2(p.x + v.x, p.y + v.y);
            a[lo + m] = make_float2(p.x - v.x, p.y - v.y);
        }
        __syncthreads();
    }

    // ---- power spectrum and the frame's energy ----
    const float inv_n = 1.0f / (float)nfft;                        // nfft is a power of two: exact
    float e = 0.0f;
    for (int k = tid; k < nbins; k += SPEECH_THREADS) {
        const float2 z = a[k];
        float p = (z.x * z.x + z.y * z.y) * inv_n;
        if (mode == NM_SPEECH_SSC && p == 0.0f) p = SPEECH_EPS;
        P[k] = p;
        e += p;
    }
    e = nm_wave_sum(e);
    if (lane == 0) red[wave] = e;
    __syncthreads();
    const float energy = (red[0] + red[1]) + (red[2] + red[3]);    // (an exact 0 becomes eps in speech_log)

    // ---- the mel filters, a wavefront per filter over its own bins ----
    for (int j = wave; j < nfilt; j += SPEECH_THREADS / 64) {
        int k0 = fb_range[2 * j], k1 = fb_range[2 * j + 1];
        k0 = k0 < 0 ? 0 : k0;
        k1 = k1 > nbins ? nbins : k1;
        const float* frow = fb + (long)j * nbins;
        float acc = 0.0f, num = 0.0f;
        for (int k = k0 + lane; k < k1; k += 64) {
            const float pw = P[k] * frow[k];
            acc += pw;
            if (mode == NM_SPEECH_SSC) num = fmaf(P[k] * R[k], frow[k], num);
        }
        acc = nm_wave_sum(acc);
        if (mode == NM_SPEECH_SSC) num = nm_wave_sum(num);
        if (lane == 0) {
            F[j] = acc;
            G[j] = num;
        }
    }
    __syncthreads();

    // ---- the row ----
    if (mode == NM_SPEECH_FBANK) {
        for (int j = tid; j < nfilt; j += SPEECH_THREADS) orow[j] = F[j] == 0.0f ? SPEECH_EPS : F[j];
    } else if (mode == NM_SPEECH_LOGFBANK) {
        for (int j = tid; j < nfilt; j += SPEECH_THREADS) orow[j] = speech_log(F[j]);
    } else if (mode == NM_SPEECH_SSC) {
        for (int j = tid; j < nfilt; j += SPEECH_THREADS) orow[j] = G[j] / F[j];
    } else {
        for (int j = tid; j < nfilt; j += SPEECH_THREADS) G[j] = speech_log(F[j]);
        __syncthreads();
        for (int c = tid; c < numcep; c += SPEECH_THREADS) {
            const float* drow = dct + (long)c * nfilt;
            float acc = 0.0f;
            for (int j = 0; j < nfilt; ++j) acc = fmaf(drow[j], G[j], acc);
            orow[c] = (c == 0 && append_energy) ? speech_log(energy) : acc;
        }
    }
}

__global__ __launch_bounds__(SPEECH_THREADS) void speech_deltas_kernel(float* out, long ld,
                                                                       const int64_t* __restrict__ frame_off, long U,
                                                                       long total_frames, int F, long order, int N,
                                                                       float denom) {
    const long e = (long)blockIdx.x * SPEECH_THREADS + threadIdx.x;
    if (e >= total_frames * F) return;
    const long row = e / F;
    const int c = (int)(e - row * F);
    float* dst = out + row * ld + (order + 1) * F + c;
    const long u = speech_owner(frame_off, U, row);
    long f0 = frame_off[u], f1 = frame_off[u + 1];
    f0 = f0 < 0 ? 0 : f0;
    f1 = f1 > total_frames ? total_frames : f1;
    if (row < f0 || row >= f1) {
        *dst = 0.0f;
        return;
    }
    const float* src = out + order * F + c;
    float acc = 0.0f;
    for (int i = -N; i <= N; ++i) {
        long r = row + i;
        r = r < f0 ? f0 : (r > f1 - 1 ? f1 - 1 : r);
        acc = fmaf((float)i, src[r * ld], acc);
    }
    *dst = acc / denom;
}

size_t speech_lds_bytes(int64_t nfft, int64_t nfilt) {
    const int64_t nbins = nfft / 2 + 1;
    return (size_t)nfft * sizeof(float2) + (size_t)(((nbins + 3) & ~3ll) + 2 * ((nfilt + 3) & ~3ll) + 4) * sizeof(float);
}

}  // namespace

extern "C" {

int nm_speech_frames(void* stream, const float* wav, const int64_t* sample_off, const int64_t* frame_off, int64_t U,
                     int64_t total_samples, int64_t total_frames, int64_t fl, int64_t fs, int64_t nfft, float preemph,
                     const float* window, const float* twiddles, const float* fb, const int32_t* fb_range, int64_t nfilt,
                     const float* dct, int64_t numcep, const float* R, int mode, int append_energy, float* out,
                     int64_t ld) {
    NM_REQUIRE(U >= 1, "nm_speech_frames: U = %lld utterances, at least 1 is needed", (long long)U);
    NM_REQUIRE(total_samples >= 0, "nm_speech_frames: total_samples %lld", (long long)total_samples);
    NM_REQUIRE(total_frames >= 0 && total_frames <= (1ll << 31) - 1,
               "nm_speech_frames: total_frames %lld outside 0 .. 2^31 - 1", (long long)total_frames);
    NM_REQUIRE(fl >= 1 && fs >= 1, "nm_speech_frames: frame length %lld and step %lld must be at least 1", (long long)fl,
               (long long)fs);
    NM_REQUIRE(nfft >= NM_SPEECH_MIN_NFFT && nfft <= NM_SPEECH_MAX_NFFT && (nfft & (nfft - 1)) == 0,
               "nm_speech_frames: nfft %lld is not a power of two in %d..%d", (long long)nfft, NM_SPEECH_MIN_NFFT,
               NM_SPEECH_MAX_NFFT);
    NM_REQUIRE(nfilt >= 1 && nfilt <= NM_SPEECH_MAX_NFILT, "nm_speech_frames: nfilt %lld outside 1..%d", (long long)nfilt,
               NM_SPEECH_MAX_NFILT);
    NM_REQUIRE(mode >= NM_SPEECH_MFCC && mode <= NM_SPEECH_SSC, "nm_speech_frames: unknown mode %d", mode);
    NM_REQUIRE(mode != NM_SPEECH_MFCC || (numcep >= 1 && numcep <= nfilt),
               "nm_speech_frames: numcep %lld outside 1..nfilt = %lld", (long long)numcep, (long long)nfilt);
    const int64_t width = mode == NM_SPEECH_MFCC ? numcep : nfilt;
    NM_REQUIRE(ld >= width, "nm_speech_frames: ld %lld below the block's width %lld", (long long)ld, (long long)width);
    if (total_frames == 0) return NM_OK;
    NM_REQUIRE(sample_off != nullptr && frame_off != nullptr && window != nullptr && twiddles != nullptr &&
                   fb != nullptr && fb_range != nullptr && out != nullptr && (wav != nullptr || total_samples == 0),
               "nm_speech_frames: null pointer (wav, sample_off, frame_off, window, twiddles, fb, fb_range or out)");
    NM_REQUIRE(mode != NM_SPEECH_MFCC || dct != nullptr, "nm_speech_frames: null dct in MFCC mode");
    NM_REQUIRE(mode != NM_SPEECH_SSC || R != nullptr, "nm_speech_frames: null R in SSC mode");
    int log2n = 0;
    while ((1ll << log2n) < nfft) ++log2n;
    hipLaunchKernelGGL(speech_frames_kernel, dim3((unsigned)total_frames), dim3(SPEECH_THREADS),
                       speech_lds_bytes(nfft, nfilt), nm_stream(stream), wav, sample_off, frame_off, (long)U,
                       (long)total_samples, (long)total_frames, (long)fl, (long)fs, (int)nfft, log2n, preemph, window,
                       reinterpret_cast<const float2*>(twiddles), fb, fb_range, (int)nfilt, dct, (int)numcep, R, mode,
                       append_energy ? 1 : 0, out, (long)ld);
    NM_LAUNCH_CHECK("nm_speech_frames");
}

int nm_speech_deltas(void* stream, float* out, int64_t ld, const int64_t* frame_off, int64_t U, int64_t total_frames,
                     int64_t F, int64_t order, int64_t N) {
    NM_REQUIRE(U >= 1, "nm_speech_deltas: U = %lld utterances, at least 1 is needed", (long long)U);
    NM_REQUIRE(total_frames >= 0 && total_frames <= (1ll << 31) - 1,
               "nm_speech_deltas: total_frames %lld outside 0 .. 2^31 - 1", (long long)total_frames);
    NM_REQUIRE(F >= 1 && F <= (1 << 20), "nm_speech_deltas: block width F %lld outside 1..2^20", (long long)F);
    NM_REQUIRE(order >= 0 && order <= 1024, "nm_speech_deltas: order %lld outside 0..1024", (long long)order);
    NM_REQUIRE(N >= 1 && N <= NM_SPEECH_MAX_DELTA_WINDOW, "nm_speech_deltas: window N %lld outside 1..%d", (long long)N,
               NM_SPEECH_MAX_DELTA_WINDOW);
    NM_REQUIRE(ld >= (order + 2) * F, "nm_speech_deltas: ld %lld below (order + 2) * F = %lld", (long long)ld,
               (long long)((order + 2) * F));
    if (total_frames == 0) return NM_OK;
    NM_REQUIRE(out != nullptr && frame_off != nullptr, "nm_speech_deltas: null pointer (out or frame_off)");
    const int64_t blocks = (total_frames * F + SPEECH_THREADS - 1) / SPEECH_THREADS;
    NM_REQUIRE(blocks <= (1ll << 31) - 1, "nm_speech_deltas: total_frames * F = %lld elements beyond one grid",
               (long long)(total_frames * F));
    float denom = 0.0f;
    for (int64_t i = 1; i <= N; ++i) denom += 2.0f * (float)(i * i);
    hipLaunchKernelGGL(speech_deltas_kernel, dim3((unsigned)blocks), dim3(SPEECH_THREADS), 0, nm_stream(stream), out,
                       (long)ld, frame_off, (long)U, (long)total_frames, (int)F, (long)order, (int)N, denom);
    NM_LAUNCH_CHECK("nm_speech_deltas");
}

}  // extern "C"
