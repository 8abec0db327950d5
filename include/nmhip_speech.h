/* libnmhip -- C ABI of the speech front end (csrc/nm_speech.hip), a companion of nmhip.h with the same conventions: every
 * function returns 0 on success, <0 on error with the text in nm_last_error(); pointers are DEVICE pointers owned by the
 * caller; `stream` is a hipStream_t passed as void*; sizes are int64_t element counts.  Arguments are checked before
 * anything is launched.  No atomics: two runs are bit-equal, and an utterance's rows do not depend on what else is in
 * the batch.
 *
 * The arithmetic is the published algorithm of python_speech_features 0.6 (mfcc, fbank, logfbank, ssc, delta), which
 * the reference's processors/speech.py delegates to, in fp32.  A ragged batch of U utterances is one array of samples
 * with U + 1 offsets; the features of all of them are the rows of one output [total_frames, ld] with U + 1 row offsets.
 * The host converts integer PCM to fp32 once: int16 and uint8 samples are exact in fp32, int32 samples are ROUNDED to
 * 24 bits.  Every table below is made on the host in float64 and rounded once. */
#ifndef NMHIP_SPEECH_H
#define NMHIP_SPEECH_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define NM_SPEECH_MFCC 0
#define NM_SPEECH_FBANK 1
#define NM_SPEECH_LOGFBANK 2
#define NM_SPEECH_SSC 3
#define NM_SPEECH_MAX_NFFT 4096
#define NM_SPEECH_MIN_NFFT 64
#define NM_SPEECH_MAX_NFILT 256
#define NM_SPEECH_MAX_DELTA_WINDOW 64

/* Feature block 0 of every frame, one workgroup per frame.  Frame t of utterance u is output row frame_off[u] + t and
 * reads the samples y[t*fs + i] * window[i], i < min(fl, nfft), of the utterance's pre-emphasised signal
 *   y[0] = x[0], y[i] = x[i] - preemph * x[i-1]  (x = wav[sample_off[u] .. sample_off[u+1])), zero past the utterance's end
 * (so the first sample of the UTTERANCE is the one copied through); the rest of the nfft points are zero.  Then
 *   P[k] = |fft(frame)[k]|^2 / nfft, k = 0 .. nfft/2       E = sum_k P[k], eps where exactly 0 (eps = 2^-52)
 *   F[j] = sum_k P[k] * fb[j*(nfft/2+1) + k] over k in [fb_range[2j], fb_range[2j+1]), eps where exactly 0
 *   mode FBANK     out[row, j] = F[j]                                                       j < nfilt
 *   mode LOGFBANK  out[row, j] = log F[j]
 *   mode MFCC      out[row, c] = sum_j dct[c*nfilt + j] * log F[j], c < numcep; with append_energy, out[row, 0] = log E
 *   mode SSC       P's exact zeros become eps first; out[row, j] = sum_k P[k] R[k] fb[j,k] / sum_k P[k] fb[j,k]
 * log(eps) is stored as the constant float(log(2^-52)).  twiddles: nfft/2 pairs (cos, -sin)(2 pi k / nfft).
 * dct: the orthonormal DCT-II rows with the lifter folded in (MFCC only, else ignored); R: [nfft/2+1] (SSC only).
 * Offsets are read on the device and never trusted: a sample index outside [0, total_samples) or outside its utterance
 * reads as 0, bin ranges are clamped to [0, nfft/2], and a row that no utterance owns is written as zeros.
 * Refused: null wav (with samples), sample_off, frame_off, window, twiddles, fb, fb_range or out; null dct for MFCC,
 * null R for SSC; U < 1; total_samples < 0; total_frames < 0 or beyond 2^31 - 1; fl < 1; fs < 1; nfft not a power of
 * two in 64..4096; nfilt outside 1..256; MFCC with numcep outside 1..nfilt; an unknown mode; ld below the block's width
 * (numcep for MFCC, else nfilt).  total_frames == 0 is a no-op. */
int nm_speech_frames(void* stream, const float* wav, const int64_t* sample_off, const int64_t* frame_off, int64_t U,
                     int64_t total_samples, int64_t total_frames, int64_t fl, int64_t fs, int64_t nfft, float preemph,
                     const float* window, const float* twiddles, const float* fb, const int32_t* fb_range, int64_t nfilt,
                     const float* dct, int64_t numcep, const float* R, int mode, int append_energy, float* out,
                     int64_t ld);

/* One order of deltas, from column block `order` to column block `order + 1` of out [total_frames, ld], blocks F wide:
 *   out[r, (order+1)*F + c] = sum_{i=-N..N} i * out[clamp(r + i), order*F + c] / (2 * sum_{i=1..N} i^2)
 * with the row clamped to the rows [frame_off[u], frame_off[u+1]) of r's own utterance.  A second launch, not a fused
 * one: a row reads 2N + 1 rows of the block before.
 * Refused: null out or frame_off; U < 1; total_frames < 0 or beyond 2^31 - 1; F < 1; order < 0; N outside 1..64;
 * ld < (order + 2) * F.  total_frames == 0 is a no-op. */
int nm_speech_deltas(void* stream, float* out, int64_t ld, const int64_t* frame_off, int64_t U, int64_t total_frames,
                     int64_t F, int64_t order, int64_t N);

#ifdef __cplusplus
}
#endif
#endif
