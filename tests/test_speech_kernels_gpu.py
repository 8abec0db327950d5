"""The two kernels of csrc/nm_speech.hip on the MI355X, through ``SpeechFeaturesPreprocessor`` -> ops -> the C ABI, against
the float64 restatement of python_speech_features' algorithm in tests/speech_ref.py, on the smallest inputs where each
stage can break.

Tolerance.  fp32 against float64 is not derivable for these features: a frame in near-silence loses digits to
cancellation before the ``log``.  So every case computes the restatement twice, in float64 (the reference) and on fp32
arrays (a second evaluation of the reference, not of the code under test), and the kernels' error must stay within 8
times the fp32 restatement's largest error on that same input, with a floor of 1e-5 -- the factor allows for another
summation order in the transform.  ``mfcc`` and ``logfbank`` are compared absolutely, the linear ``fbank`` and ``ssc``
relatively by the same rule; values of the eps branch are compared exactly.  Every case prints its figures before it
asserts; DESIGN 4.18 records them."""
import os
import warnings

import numpy as np
import pytest

from . import speech_ref as R
from .test_speech_host import YESNO, audio_root  # noqa: F401  pylint: disable=unused-import

pytestmark = pytest.mark.gpu

LOG_KINDS = ("mfcc", "logfbank")
FACTOR, FLOOR = 8.0, 1e-5


def tone(samples, rate, seed=0, dtype=np.int16):
    """Two tones and a little noise, as integer PCM."""
    rng = np.random.RandomState(seed)
    t = np.arange(samples) / rate
    wave = 3000 * np.sin(2 * np.pi * 440 * t) + 1500 * np.sin(2 * np.pi * 0.21 * rate * t + 1) + rng.randn(samples) * 200
    if dtype == np.uint8:
        return np.clip(wave / 40 + 128, 0, 255).astype(np.uint8)
    return wave.astype(dtype)


def preprocessor(kind="mfcc", delta_order=0, delta_window=2, **kwargs):
    from neuralmonkey_amd.processors.speech import SpeechFeaturesPreprocessor
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return SpeechFeaturesPreprocessor(kind, delta_order, delta_window, **kwargs)


def check(got, signal, rate, kind="mfcc", delta_order=0, delta_window=2, label="", **kwargs):
    """``got`` against the float64 restatement under the module's tolerance rule; returns (error, bound)."""
    args = dict(feature_type=kind, delta_order=delta_order, delta_window=delta_window, **kwargs)
    ref = R.features(signal, rate, dtype=np.float64, **args)
    again = R.features(signal, rate, dtype=np.float32, **args).astype(np.float64)
    assert got.dtype == np.float32 and got.shape == ref.shape, (got.shape, ref.shape)
    width = ref.shape[1] // (delta_order + 1)
    # the eps branch (feature block 0 only): exact
    exact = np.zeros(ref.shape, bool)
    if kind == "fbank":
        exact[:, :width] = ref[:, :width] == R.EPS
    elif kind == "logfbank":
        exact[:, :width] = ref[:, :width] == np.log(R.EPS)
    elif kind == "mfcc" and kwargs.get("appendEnergy", True):
        exact[:, 0] = ref[:, 0] == np.log(R.EPS)
    assert np.array_equal(got[exact], ref[exact].astype(np.float32)), label
    rest = ~exact
    if not rest.any():
        print("speech {:<40} eps branch only ({} values exact)".format(label, exact.sum()))
        return 0.0, FLOOR
    assert np.isfinite(got[rest]).all(), label
    scale = 1.0 if kind in LOG_KINDS else np.abs(ref[rest])
    own = float(np.max(np.abs(again[rest] - ref[rest]) / scale))
    err = float(np.max(np.abs(got[rest].astype(np.float64) - ref[rest]) / scale))
    bound = max(FACTOR * own, FLOOR)
    print("speech {:<40} kernel {:.3e}  fp32 restatement {:.3e}  bound {:.3e}  ({} eps values exact)".format(
        label, err, own, bound, int(exact.sum())))
    assert err <= bound, (label, err, bound)
    return err, bound


def run(signal, rate, kind="mfcc", delta_order=0, delta_window=2, label="", **kwargs):
    from neuralmonkey_amd.readers.audio_reader import Audio
    got = preprocessor(kind, delta_order, delta_window, **kwargs)(Audio(rate, signal))
    return check(got, signal, rate, kind, delta_order, delta_window, label=label, **kwargs)


@pytest.mark.parametrize("kind", ["mfcc", "fbank", "logfbank", "ssc"])
def test_utterance_lengths_around_one_frame(dev, kind):
    """Rate 8000: frames of 200 samples every 80.  50 samples are less than a frame, 201 are two frames with the second
    nearly all padding, 281 are three."""
    for samples, frames in ((50, 1), (200, 1), (201, 2), (281, 3)):
        signal = tone(samples, 8000, seed=samples)
        assert R.features(signal, 8000, kind).shape[0] == frames
        run(signal, 8000, kind, label="{} 8000 Hz, {} samples".format(kind, samples))


def test_all_zero_utterance_is_the_eps_branch_exactly(dev):
    from neuralmonkey_amd.readers.audio_reader import Audio
    silent = Audio(8000, np.zeros(300, np.int16))
    log_eps = np.float32(np.log(2.0 ** -52))
    got = preprocessor("logfbank")(silent)
    assert got.shape == (3, 26) and np.all(got == log_eps)
    got = preprocessor("mfcc")(silent)
    assert got.shape == (3, 13) and np.all(got[:, 0] == log_eps)
    check(got, silent.data, 8000, "mfcc", label="mfcc of silence")
    got = preprocessor("fbank")(silent)
    assert np.all(got == np.float32(2.0 ** -52))
    check(preprocessor("logfbank", 1)(silent), silent.data, 8000, "logfbank", 1, label="logfbank + delta of silence")
    # an empty utterance is one frame of padding
    assert np.all(preprocessor("logfbank")(Audio(8000, np.zeros(0, np.int16))) == log_eps)


@pytest.mark.parametrize("rate,samples,frames,nfft", [(8000, 700, 8, 256), (16000, 1000, 5, 512), (44100, 3000, 6, 2048)])
def test_rates_and_transform_lengths(dev, rate, samples, frames, nfft):
    pre = preprocessor("mfcc")
    assert pre.tables(rate).nfft == nfft
    for kind in ("mfcc", "ssc"):
        signal = tone(samples, rate, seed=rate)
        assert R.features(signal, rate, kind).shape[0] == frames
        run(signal, rate, kind, label="{} {} Hz nfft {}".format(kind, rate, nfft))


def test_explicit_transform_lengths_and_the_truncated_frame(dev):
    from neuralmonkey_amd.processors.speech import SpeechFeaturesPreprocessor
    from neuralmonkey_amd.readers.audio_reader import Audio
    signal = tone(1000, 16000, seed=4)
    run(signal, 16000, "mfcc", nfft=512, label="mfcc fl 400 nfft 512")
    run(signal, 16000, "logfbank", nfft=1024, label="logfbank fl 400 nfft 1024")
    run(tone(1000, 8000, seed=5), 8000, "logfbank", nfft=4096, label="logfbank fl 200 nfft 4096")
    run(tone(300, 8000, seed=6), 8000, "fbank", nfft=64, winlen=0.005, label="fbank fl 40 nfft 64")
    with pytest.warns(UserWarning, match=r"frame length \(400\) is greater than FFT size \(256\)"):
        got = SpeechFeaturesPreprocessor("mfcc", nfft=256)(Audio(16000, signal))
    check(got, signal, 16000, "mfcc", nfft=256, label="mfcc fl 400 nfft 256 (truncated)")


@pytest.mark.parametrize("name,rate,kwargs", [
    ("nfilt 40 numcep 20", 16000, dict(nfilt=40, numcep=20)),
    ("ceplifter 0", 8000, dict(ceplifter=0)),
    ("appendEnergy False", 8000, dict(appendEnergy=False)),
    ("preemph 0", 8000, dict(preemph=0)),
    ("lowfreq 100 highfreq 3000", 8000, dict(lowfreq=100, highfreq=3000)),
    ("winfunc hamming", 8000, dict(winfunc=np.hamming)),
    ("winlen 0.02 winstep 0.005", 16000, dict(winlen=0.02, winstep=0.005))])
def test_non_default_parameters(dev, name, rate, kwargs):
    run(tone(rate // 10, rate, seed=len(name)), rate, "mfcc", label="mfcc " + name, **kwargs)
    if "numcep" not in kwargs and "ceplifter" not in kwargs and "appendEnergy" not in kwargs:
        run(tone(rate // 10, rate, seed=len(name)), rate, "ssc", label="ssc " + name, **kwargs)


def test_integer_widths_reach_the_device_as_they_are(dev):
    run(tone(500, 8000, seed=7, dtype=np.uint8), 8000, "logfbank", label="logfbank of uint8 PCM")
    wide = tone(500, 8000, seed=8).astype(np.int32) * 65536 + 12345
    # (int32 samples are rounded to fp32 on the host: the reference here is the restatement of the ROUNDED samples)
    from neuralmonkey_amd.readers.audio_reader import Audio
    got = preprocessor("logfbank")(Audio(8000, wide))
    check(got, wide.astype(np.float32).astype(np.float64), 8000, "logfbank", label="logfbank of int32 PCM")


@pytest.mark.parametrize("samples,frames", [(150, 1), (250, 2), (680, 7)])
@pytest.mark.parametrize("order", [0, 1, 2])
def test_deltas_with_clamped_edges(dev, samples, frames, order):
    """Windows 1, 2 and 3 on 1, 2 and 7 frames: with fewer frames than the window every term is clamped."""
    signal = tone(samples, 8000, seed=samples + order)
    for window in (1, 2, 3):
        for kind in ("mfcc", "logfbank"):
            assert R.features(signal, 8000, kind, order, window).shape == (frames, (13 if kind == "mfcc" else 26) * (order + 1))
            run(signal, 8000, kind, order, window, label="{} {} frames order {} window {}".format(kind, frames, order, window))


def test_ragged_batch_is_bit_equal_to_single_calls_and_to_a_second_run(dev):
    from neuralmonkey_amd.readers.audio_reader import Audio
    audios = [Audio(8000, tone(150, 8000, seed=1)), Audio(8000, tone(680, 8000, seed=2)), Audio(8000, tone(360, 8000, seed=3))]
    # (ssc without deltas: a linear feature is compared relatively, which deltas near 0 do not allow)
    for kind, order in (("mfcc", 2), ("ssc", 0)):
        pre = preprocessor(kind, order, 3)
        together = pre.many(audios)
        assert [a.shape[0] for a in together] == [1, 7, 3]
        singles = [pre(audio) for audio in audios]
        second = pre.many(audios)
        for a, b, c, audio in zip(together, singles, second, audios):
            assert np.array_equal(a, b) and np.array_equal(a, c)
            check(a, audio.data, 8000, kind, order, 3, label="{} ragged, {} samples".format(kind, len(audio.data)))
    # two sample rates in one list: a pair of launches per rate, the list's order kept
    pre = preprocessor("mfcc", 1)
    mixed = [audios[1], Audio(16000, tone(1000, 16000, seed=9)), audios[0]]
    for got, audio in zip(pre.many(mixed), mixed):
        assert np.array_equal(got, pre(audio))


def test_real_recordings(dev, audio_root):  # noqa: F811
    from neuralmonkey_amd.readers.audio_reader import read_wav
    names = ["tests/data/dtmf/test_2.wav", "tests/data/dtmf/8.wav", "tests/data/dtmf/5.wav", YESNO]
    audios = [read_wav(os.path.join(audio_root, name)) for name in names]
    assert [len(a.data) for a in audios] == [3612, 7882, 10644, 50400]
    for kind, order in (("mfcc", 2), ("logfbank", 0)):
        pre = preprocessor(kind, order)
        for name, audio, got in zip(names, audios, pre.many(audios)):
            check(got, audio.data, audio.rate, kind, order, label="{} {}".format(kind, os.path.basename(name)))
    assert pre.many(audios[:1])[0].shape == (7, 26)
