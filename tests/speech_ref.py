"""NumPy restatement of the speech features the reference computes with ``python_speech_features`` 0.6 (``mfcc``,
``fbank``, ``logfbank``, ``ssc``, ``delta``), written from that package's published algorithm; what the tests of the
device kernels (csrc/nm_speech.hip) compare against.

``python_speech_features`` itself is installed on neither the build machine nor the GPU machine, so parity rests on THIS
restatement of its algorithm, not on recorded output of the package.  Where the package is available, a recorded
fixture under tests/golden/ can be added beside it.  One default differs from the package's, as the engine's does
(DESIGN 4.18): ``nfft=None`` -- derived from ``winlen * rate`` -- for every function here, where the package's ``fbank``,
``logfbank`` and ``ssc`` default to ``nfft=512`` and only its ``mfcc`` to ``None``.

Every function takes ``dtype``: ``np.float64`` is the reference; ``np.float32`` runs the same statements on fp32 arrays
(``numpy.fft`` of NumPy 2 transforms fp32 frames in fp32; an older NumPy transforms them in float64, and its result is
rounded to fp32) -- a second evaluation of the reference whose distance from the first measures how many digits the
features keep in fp32, which is what bounds the kernels' error in the tests."""
import decimal
import math

import numpy as np

EPS = 2.220446049250313e-16          # numpy.finfo(float).eps = 2^-52, exact in fp32


def round_half_up(number):
    return int(decimal.Decimal(number).quantize(decimal.Decimal("1"), rounding=decimal.ROUND_HALF_UP))


def default_nfft(rate, winlen):
    nfft = 1
    while nfft < winlen * rate:
        nfft *= 2
    return nfft


def framing(rate, winlen=0.025, winstep=0.01, nfft=None):
    """(frame length, frame step, transform length)."""
    return round_half_up(winlen * rate), round_half_up(winstep * rate), nfft or default_nfft(rate, winlen)


def num_frames(samples, frame_len, frame_step):
    if samples <= frame_len:
        return 1
    return 1 + int(math.ceil((1.0 * samples - frame_len) / frame_step))


def frames_of(signal, frame_len, frame_step, window, dtype):
    count = num_frames(len(signal), frame_len, frame_step)
    padded = np.zeros((count - 1) * frame_step + frame_len, dtype)
    padded[:len(signal)] = signal
    index = np.arange(frame_len)[None, :] + (np.arange(count) * frame_step)[:, None]
    return padded[index] * window.astype(dtype)[None, :]


def power_spectrum(frames, nfft, dtype):
    """|rfft|^2 / nfft; frames longer than nfft are truncated (the package warns and does the same)."""
    spectrum = np.fft.rfft(frames, nfft)
    real, imag = spectrum.real.astype(dtype), spectrum.imag.astype(dtype)
    return (real * real + imag * imag) * dtype(1.0 / nfft)


def hz2mel(hz):
    return 2595 * np.log10(1 + hz / 700.)


def mel2hz(mel):
    return 700 * (10 ** (mel / 2595.0) - 1)


def filterbank(nfilt, nfft, rate, lowfreq, highfreq):
    highfreq = highfreq or rate / 2
    assert highfreq <= rate / 2
    points = np.linspace(hz2mel(lowfreq), hz2mel(highfreq), nfilt + 2)
    edges = np.floor((nfft + 1) * mel2hz(points) / rate)
    bank = np.zeros([nfilt, nfft // 2 + 1])
    for j in range(nfilt):
        for i in range(int(edges[j]), int(edges[j + 1])):
            bank[j, i] = (i - edges[j]) / (edges[j + 1] - edges[j])
        for i in range(int(edges[j + 1]), int(edges[j + 2])):
            bank[j, i] = (edges[j + 2] - i) / (edges[j + 2] - edges[j + 1])
    return bank


def dct_matrix(numcep, nfilt):
    """Rows of the orthonormal DCT-II (what scipy.fftpack.dct(type=2, norm="ortho") multiplies by)."""
    c, j = np.arange(numcep)[:, None], np.arange(nfilt)[None, :]
    matrix = np.sqrt(2.0 / nfilt) * np.cos(np.pi * c * (2 * j + 1) / (2.0 * nfilt))
    matrix[0] /= np.sqrt(2.0)
    return matrix


def spectrum_of(signal, rate, winlen, winstep, nfft, preemph, winfunc, dtype):
    signal = np.asarray(signal).astype(dtype)
    frame_len, frame_step, nfft = framing(rate, winlen, winstep, nfft)
    emphasised = np.append(signal[:1], signal[1:] - dtype(preemph) * signal[:-1]) if len(signal) else signal
    window = np.ones(frame_len) if winfunc is None else np.asarray(winfunc(frame_len), np.float64)
    return power_spectrum(frames_of(emphasised, frame_len, frame_step, window, dtype), nfft, dtype), nfft


def fbank(signal, rate, winlen=0.025, winstep=0.01, nfilt=26, nfft=None, lowfreq=0, highfreq=None, preemph=0.97,
          winfunc=None, dtype=np.float64):
    """(filterbank energies [frames, nfilt], frame energies [frames]), exact zeros replaced by eps."""
    pspec, nfft = spectrum_of(signal, rate, winlen, winstep, nfft, preemph, winfunc, dtype)
    energy = np.sum(pspec, 1)
    energy = np.where(energy == 0, dtype(EPS), energy)
    feat = np.dot(pspec, filterbank(nfilt, nfft, rate, lowfreq, highfreq).astype(dtype).T)
    return np.where(feat == 0, dtype(EPS), feat), energy


def logfbank(signal, rate, dtype=np.float64, **kwargs):
    return np.log(fbank(signal, rate, dtype=dtype, **kwargs)[0])


def mfcc(signal, rate, numcep=13, ceplifter=22, appendEnergy=True, dtype=np.float64, **kwargs):          # pylint: disable=invalid-name
    feat, energy = fbank(signal, rate, dtype=dtype, **kwargs)
    nfilt = feat.shape[1]
    assert numcep <= nfilt
    feat = np.dot(np.log(feat), dct_matrix(numcep, nfilt).astype(dtype).T)
    if ceplifter > 0:
        feat = feat * (1 + (ceplifter / 2.) * np.sin(np.pi * np.arange(numcep) / ceplifter)).astype(dtype)[None, :]
    if appendEnergy:
        feat[:, 0] = np.log(energy)
    return feat


def ssc(signal, rate, winlen=0.025, winstep=0.01, nfilt=26, nfft=None, lowfreq=0, highfreq=None, preemph=0.97,
        winfunc=None, dtype=np.float64):
    pspec, nfft = spectrum_of(signal, rate, winlen, winstep, nfft, preemph, winfunc, dtype)
    pspec = np.where(pspec == 0, dtype(EPS), pspec)
    bank = filterbank(nfilt, nfft, rate, lowfreq, highfreq).astype(dtype)
    freqs = np.linspace(1, rate / 2, pspec.shape[1]).astype(dtype)
    return np.dot(pspec * freqs[None, :], bank.T) / np.dot(pspec, bank.T)


def delta(feat, window):
    assert window >= 1
    denominator = 2 * sum(i ** 2 for i in range(1, window + 1))
    count = len(feat)
    out = np.zeros_like(feat)
    for t in range(count):
        for i in range(-window, window + 1):
            out[t] += feat.dtype.type(i) * feat[min(max(t + i, 0), count - 1)]
    return out / feat.dtype.type(denominator)


FEATURES = {"mfcc": mfcc, "fbank": lambda *a, **k: fbank(*a, **k)[0], "logfbank": logfbank, "ssc": ssc}


def features(signal, rate, feature_type="mfcc", delta_order=0, delta_window=2, dtype=np.float64, **kwargs):
    """What ``SpeechFeaturesPreprocessor(feature_type, delta_order, delta_window, **kwargs)`` returns for one utterance."""
    blocks = [FEATURES[feature_type](signal, rate, dtype=dtype, **kwargs)]
    for _ in range(delta_order):
        blocks.append(delta(blocks[-1], delta_window))
    return np.concatenate(blocks, axis=1)
