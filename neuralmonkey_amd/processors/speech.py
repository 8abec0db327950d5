"""Speech features on the device (interface of neuralmonkey/processors/speech.py).

The reference hands the arithmetic to the third-party ``python_speech_features`` package (``mfcc``, ``fbank``,
``logfbank``, ``ssc``, ``delta``).  This engine contains it: framing, pre-emphasis, FFT, mel filters, DCT, lifter and
deltas of that package's version 0.6 run in two HIP kernels (csrc/nm_speech.hip, include/nmhip_speech.h) over a ragged
batch of utterances; nothing is computed on the host at run time except the tables below, once per sample rate.

``SpeechFeaturesPreprocessor(...)`` returns a callable object: ``obj(audio)`` is the float32 array
``[frames, F * (delta_order + 1)]`` of one ``Audio``; ``obj.many(list of Audio)`` is the list of such arrays, computed
over all of them at once -- one launch for the features and one per delta order, whatever the number of utterances;
``dataset.load`` feeds it chunks of a series.

Engine decisions: the transform length is a power of two in 64..4096, given or derived; at most 256
filters; only one channel; the keyword arguments are checked when the object is built, not at the first utterance."""
import decimal
import math
import warnings
from typing import Any, Dict, List

import numpy as np

from ..readers.audio_reader import Audio

FEATURE_TYPES = {"mfcc": 0, "fbank": 1, "logfbank": 2, "ssc": 3}          # the mode flags of include/nmhip_speech.h
COMMON_KWARGS = {"winlen": 0.025, "winstep": 0.01, "nfilt": 26, "nfft": None, "lowfreq": 0, "highfreq": None,
                 "preemph": 0.97, "winfunc": None}
MFCC_KWARGS = {"numcep": 13, "ceplifter": 22, "appendEnergy": True}
MIN_NFFT, MAX_NFFT, MAX_NFILT, MAX_DELTA_WINDOW = 64, 4096, 256, 64


def round_half_up(number: float) -> int:
    return int(decimal.Decimal(number).quantize(decimal.Decimal("1"), rounding=decimal.ROUND_HALF_UP))


def frame_count(samples: int, frame_len: int, frame_step: int) -> int:
    if samples <= frame_len:
        return 1
    return 1 + int(math.ceil((1.0 * samples - frame_len) / frame_step))


def hz2mel(hz):
    return 2595 * np.log10(1 + hz / 700.)


def mel2hz(mel):
    return 700 * (10 ** (mel / 2595.0) - 1)


class SpeechTables:
    """What the kernels read for one sample rate: sizes, and the float64-made tables rounded once to fp32."""

    def __init__(self, rate: int, opts: Dict[str, Any], feature_type: str) -> None:
        self.rate = rate
        self.frame_len = round_half_up(opts["winlen"] * rate)
        self.frame_step = round_half_up(opts["winstep"] * rate)
        if self.frame_len < 1 or self.frame_step < 1:
            raise ValueError("winlen {} and winstep {} give frames of {} samples every {} at {} Hz".format(
                opts["winlen"], opts["winstep"], self.frame_len, self.frame_step, rate))
        nfft = opts["nfft"]
        if nfft is None:
            nfft = 1
            while nfft < opts["winlen"] * rate:
                nfft *= 2
            if not MIN_NFFT <= nfft <= MAX_NFFT:
                raise ValueError("winlen {} at {} Hz needs nfft = {}: this engine transforms {}..{} points".format(
                    opts["winlen"], rate, nfft, MIN_NFFT, MAX_NFFT))
        self.nfft = nfft
        if self.frame_len > nfft:
            warnings.warn("frame length ({}) is greater than FFT size ({}), frame will be truncated. Increase NFFT to "
                          "avoid.".format(self.frame_len, nfft))
        highfreq = opts["highfreq"] if opts["highfreq"] is not None else rate / 2
        if highfreq > rate / 2:
            raise ValueError("highfreq is greater than samplerate/2")
        nfilt, nbins = opts["nfilt"], nfft // 2 + 1
        self.nfilt, self.nbins = nfilt, nbins
        self.preemph = float(opts["preemph"])
        window = np.ones(self.frame_len) if opts["winfunc"] is None else np.asarray(opts["winfunc"](self.frame_len),
                                                                                  np.float64)
        if window.shape != (self.frame_len,):
            raise ValueError("winfunc({}) returned an array of shape {}".format(self.frame_len, window.shape))
        self.window = window.astype(np.float32)
        angle = 2.0 * np.pi * np.arange(nfft // 2) / nfft
        self.twiddles = np.stack([np.cos(angle), -np.sin(angle)], axis=1).astype(np.float32)
        # the mel filters: nfilt + 2 points equally spaced in mel, floored to transform bins
        points = mel2hz(np.linspace(hz2mel(opts["lowfreq"]), hz2mel(highfreq), nfilt + 2))
        edges = np.floor((nfft + 1) * points / rate)
        bank = np.zeros([nfilt, nbins])
        for j in range(nfilt):
            for i in range(int(edges[j]), int(edges[j + 1])):
                bank[j, i] = (i - edges[j]) / (edges[j + 1] - edges[j])
            for i in range(int(edges[j + 1]), int(edges[j + 2])):
                bank[j, i] = (edges[j + 2] - i) / (edges[j + 2] - edges[j + 1])
        self.bank = bank.astype(np.float32)
        self.bank_range = np.zeros([nfilt, 2], np.int32)               # [first non-zero bin, one past the last)
        for j in range(nfilt):
            nonzero = np.flatnonzero(self.bank[j])
            if nonzero.size:
                self.bank_range[j] = nonzero[0], nonzero[-1] + 1
        self.dct = None
        self.numcep = 0
        self.append_energy = False
        if feature_type == "mfcc":
            numcep, lifter = opts["numcep"], opts["ceplifter"]
            self.numcep, self.append_energy = numcep, bool(opts["appendEnergy"])
            c, j = np.arange(numcep)[:, None], np.arange(nfilt)[None, :]
            dct = np.cos(np.pi * c * (2 * j + 1) / (2.0 * nfilt)) * np.sqrt(2.0 / nfilt)
            dct[0] *= np.sqrt(0.5)
            if lifter > 0:
                dct *= 1 + (lifter / 2.) * np.sin(np.pi * c / lifter)
            self.dct = dct.astype(np.float32)
        self.centroid_freqs = np.linspace(1, rate / 2, nbins).astype(np.float32) if feature_type == "ssc" else None
        self.width = self.numcep if feature_type == "mfcc" else nfilt
        self._device: Dict[Any, Dict[str, Any]] = {}

    def on_device(self, device) -> Dict[str, Any]:
        import torch
        key = str(device)
        if key not in self._device:
            self._device[key] = {name: None if array is None else torch.from_numpy(array).to(device)
                                 for name, array in (("window", self.window), ("twiddles", self.twiddles),
                                                     ("bank", self.bank), ("bank_range", self.bank_range),
                                                     ("dct", self.dct), ("centroid_freqs", self.centroid_freqs))}
        return self._device[key]


# pylint: disable=too-few-public-methods
class SpeechFeaturesPreprocessor:
    """A series-level preprocessor from ``Audio`` to a float32 array ``[frames, F * (delta_order + 1)]``.

    ``feature_type`` names the feature block: "mfcc" (F = numcep), "fbank", "logfbank" or "ssc" (F = nfilt).
    ``delta_order`` further blocks follow it, each the delta filter of half-width ``delta_window`` applied to the
    block before.  The keyword arguments are those of python_speech_features 0.6's function of that name -- winlen,
    winstep, nfilt, nfft, lowfreq, highfreq, preemph, winfunc, and for "mfcc" alone numcep, ceplifter, appendEnergy --
    with the defaults of ``COMMON_KWARGS`` / ``MFCC_KWARGS``: ``nfft=None`` (derived from ``winlen * rate``) for every
    feature type, where the package's fbank, logfbank and ssc default to 512."""

    def __init__(self, feature_type: str = "mfcc", delta_order: int = 0, delta_window: int = 2, **kwargs) -> None:
        if feature_type not in FEATURE_TYPES:
            raise ValueError("Unknown speech feature type '{}'".format(feature_type))
        accepted = dict(COMMON_KWARGS, **(MFCC_KWARGS if feature_type == "mfcc" else {}))
        for key in kwargs:
            if key not in accepted:
                raise TypeError("{}() got an unexpected keyword argument '{}'".format(feature_type, key))
        opts = dict(accepted, **kwargs)
        if delta_order < 0:
            raise ValueError("delta_order {} is negative".format(delta_order))
        if not 1 <= delta_window <= MAX_DELTA_WINDOW:
            raise ValueError("delta_window must be an integer in 1..{}, not {}".format(MAX_DELTA_WINDOW, delta_window))
        nfft = opts["nfft"]
        if nfft is not None and not (isinstance(nfft, int) and MIN_NFFT <= nfft <= MAX_NFFT and nfft & (nfft - 1) == 0):
            raise ValueError("nfft must be a power of two in {}..{}, not {!r}".format(MIN_NFFT, MAX_NFFT, nfft))
        if not 1 <= opts["nfilt"] <= MAX_NFILT:
            raise ValueError("nfilt must be in 1..{}, not {}".format(MAX_NFILT, opts["nfilt"]))
        if feature_type == "mfcc" and not 1 <= opts["numcep"] <= opts["nfilt"]:
            raise ValueError("numcep must be in 1..nfilt = {}, not {}".format(opts["nfilt"], opts["numcep"]))
        if opts["winfunc"] is not None and not callable(opts["winfunc"]):
            raise TypeError("winfunc must be a callable n -> array")
        self.feature_type = feature_type
        self.delta_order = int(delta_order)
        self.delta_window = int(delta_window)
        self.options = opts
        self._tables: Dict[int, SpeechTables] = {}

    def tables(self, rate: int) -> SpeechTables:
        """The host tables of one sample rate, made once per object (the keyword arguments never change)."""
        if rate not in self._tables:
            self._tables[rate] = SpeechTables(rate, self.options, self.feature_type)
        return self._tables[rate]

    def num_features(self, rate: int = 16000) -> int:
        return self.tables(rate).width * (self.delta_order + 1)

    def __call__(self, audio: Audio) -> np.ndarray:
        return self.many([audio])[0]

    def many(self, audios: List[Audio]) -> List[np.ndarray]:
        """The features of every utterance of the list, in its order; utterances of one sample rate share one pair of
        launches (a list with several rates takes a pair per rate)."""
        audios = list(audios)
        signals: List[np.ndarray] = []
        for audio in audios:
            data = np.asarray(audio.data)
            if data.ndim != 1:
                raise ValueError("SpeechFeaturesPreprocessor takes one channel: the audio data have shape {} "
                                 "([samples, channels])".format(tuple(data.shape)))
            signals.append(data)
        by_rate: Dict[int, List[int]] = {}
        for index, audio in enumerate(audios):
            by_rate.setdefault(int(audio.rate), []).append(index)
        plans = {rate: self.tables(rate) for rate in by_rate}                 # every refusal before any launch
        results: List[Any] = [None] * len(audios)
        for rate, members in by_rate.items():
            for index, features in zip(members, self._run(plans[rate], [signals[i] for i in members])):
                results[index] = features
        return results

    def _run(self, tab: SpeechTables, signals: List[np.ndarray]) -> List[np.ndarray]:
        import torch
        from .. import ops
        device = torch.device("cuda", torch.cuda.current_device())
        sample_off = np.zeros(len(signals) + 1, np.int64)
        frame_off = np.zeros(len(signals) + 1, np.int64)
        for u, signal in enumerate(signals):
            sample_off[u + 1] = sample_off[u] + len(signal)
            frame_off[u + 1] = frame_off[u] + frame_count(len(signal), tab.frame_len, tab.frame_step)
        wav = np.concatenate(signals).astype(np.float32) if signals else np.zeros(0, np.float32)
        out = torch.empty((int(frame_off[-1]), tab.width * (self.delta_order + 1)), dtype=torch.float32, device=device)
        d_frames = torch.from_numpy(frame_off).to(device)
        ops.speech_frames(torch.from_numpy(wav).to(device), torch.from_numpy(sample_off).to(device), d_frames,
                          tab.frame_len, tab.frame_step, tab.nfft, tab.preemph, tab.on_device(device),
                          FEATURE_TYPES[self.feature_type], tab.numcep, tab.append_energy, out)
        for order in range(self.delta_order):
            ops.speech_deltas(out, d_frames, tab.width, order, self.delta_window)
        host = out.cpu().numpy()
        return [host[frame_off[u]:frame_off[u + 1]].copy() for u in range(len(signals))]
