"""The speech front end without a GPU: the reference's two class paths through the symbol resolver, constructor signatures,
every refusal of the reader, the preprocessor and the two entry points of include/nmhip_speech.h (all of them before a
launch), the binding table, the WAV reader against scipy's, the framing arithmetic, the float64 restatement
(tests/speech_ref.py) on two committed recordings, the chunked route of ``dataset.load`` and the archive's member list."""
import ctypes
import json
import os
import re
import tarfile
import wave

import numpy as np
import pytest

from . import speech_ref
from .test_reference_inis import REF

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
BUNDLE = os.path.join(GOLDEN, "reference_tests_audio.tar.gz")
LISTS = os.path.join(GOLDEN, "speech_signatures.json")
YESNO = "tests/data/yesno/waves_yesno/0_0_1_0_0_1_1_1.wav"
# the recordings of the first four lines of train.wavlist and the first two of test.wavlist
YESNO_KEPT = ["0_0_1_0_1_0_0_0", "0_0_1_0_1_0_0_1", "0_1_0_1_0_0_0_0", "0_1_0_1_1_1_0_0", "0_0_1_0_0_1_1_1",
              "0_1_0_0_0_1_1_0"]


@pytest.fixture(scope="module")
def audio_root(tmp_path_factory):
    root = tmp_path_factory.mktemp("reference_tests_audio")
    with tarfile.open(BUNDLE) as tar:
        tar.extractall(root)
    return str(root)


# ---- the class paths ------------------------------------------------------------------------------------------------------
def test_the_references_class_paths_resolve():
    """Fails on a tree without the feature with SymbolNotShipped."""
    from neuralmonkey_amd.config.builder import resolve_symbol
    from neuralmonkey_amd.processors.speech import SpeechFeaturesPreprocessor
    from neuralmonkey_amd.readers.audio_reader import audio_reader
    assert resolve_symbol("readers.audio_reader.audio_reader") is audio_reader
    assert resolve_symbol("processors.speech.SpeechFeaturesPreprocessor") is SpeechFeaturesPreprocessor
    assert resolve_symbol("neuralmonkey.readers.audio_reader.audio_reader") is audio_reader
    assert resolve_symbol("neuralmonkey.processors.speech.SpeechFeaturesPreprocessor") is SpeechFeaturesPreprocessor


@pytest.mark.parametrize("path,name", [("readers/audio_reader.py", "audio_reader"),
                                       ("processors/speech.py", "SpeechFeaturesPreprocessor")])
def test_parameters_are_the_references(path, name):
    """As tests/test_reference_signatures.py reads them; ``**kwargs`` is no named parameter on either side."""
    from .test_reference_signatures import product_parameters, read_reference_parameters
    with open(LISTS, encoding="utf-8") as handle:
        want = [tuple(p) for p in json.load(handle)[path][name]]
    if os.path.isdir(REF):
        assert read_reference_parameters(path, name) == want
    got = product_parameters(path, name)
    if name == "SpeechFeaturesPreprocessor":
        assert got[-1] == ("kwargs", False)
        got = got[:-1]
    assert got == want


def test_audio_is_a_named_tuple():
    from neuralmonkey_amd.readers.audio_reader import Audio
    audio = Audio(8000, np.zeros(3, np.int16))
    assert audio._fields == ("rate", "data") and audio[0] == 8000 and audio.rate == 8000 and isinstance(audio, tuple)


# ---- the reader -----------------------------------------------------------------------------------------------------------
def write_wav(path, width, channels, rate, samples):
    with wave.open(str(path), "wb") as handle:
        handle.setnchannels(channels)
        handle.setsampwidth(width)
        handle.setframerate(rate)
        handle.writeframes(samples.tobytes())


def test_wav_reader_equals_scipys_on_the_committed_files(audio_root):
    from neuralmonkey_amd.readers.audio_reader import Audio, audio_reader
    data_dir = os.path.join(audio_root, "tests", "data")
    lists = [os.path.join(data_dir, "dtmf", "train.sound"), os.path.join(data_dir, "dtmf", "val.sound")]
    got = list(audio_reader(prefix=os.path.join(data_dir, "dtmf"))(lists))
    names = [line.rstrip() for path in lists for line in open(path)]
    assert len(got) == len(names) == 12 and all(isinstance(a, Audio) for a in got)
    yesno = next(iter(audio_reader(os.path.join(data_dir, "yesno"))([os.path.join(data_dir, "yesno", "test.wavlist")])))
    # sample values read here with scipy.io.wavfile.read, for machines without scipy
    assert got[0].rate == 44100 and got[0].data.dtype == np.int16 and got[0].data.shape == (18937,)
    assert got[0].data[:6].tolist() == [0, 0, -1, 2, -2, 2]
    assert yesno.rate == 8000 and yesno.data.dtype == np.int16 and yesno.data.shape == (50400,)
    assert yesno.data[:6].tolist() == [-1, 2, 1, 1, 1, 1]
    try:
        from scipy.io import wavfile
    except ImportError:
        return
    for name, audio in zip(names, got):
        rate, data = wavfile.read(os.path.join(data_dir, "dtmf", name))
        assert rate == audio.rate and data.dtype == audio.data.dtype and np.array_equal(data, audio.data), name
    rate, data = wavfile.read(os.path.join(audio_root, YESNO))
    assert rate == yesno.rate and data.dtype == yesno.data.dtype and np.array_equal(data, yesno.data)


def test_wav_reader_dtypes_and_channels(tmp_path):
    from neuralmonkey_amd.readers.audio_reader import audio_reader
    rng = np.random.RandomState(3)
    cases = {"u8.wav": (1, 1, rng.randint(0, 256, 50).astype(np.uint8)),
             "i16.wav": (2, 1, rng.randint(-32768, 32768, 50).astype("<i2")),
             "i32.wav": (4, 1, rng.randint(-2 ** 31, 2 ** 31, 50).astype("<i4")),
             "stereo.wav": (2, 2, rng.randint(-32768, 32768, (50, 2)).astype("<i2"))}
    for name, (width, channels, samples) in cases.items():
        write_wav(tmp_path / name, width, channels, 16000, samples)
    (tmp_path / "files.list").write_text("".join(name + "\n" for name in cases))
    got = list(audio_reader(prefix=str(tmp_path))([str(tmp_path / "files.list")]))
    assert [a.data.dtype for a in got] == [np.uint8, np.int16, np.int32, np.int16]
    assert [a.data.shape for a in got] == [(50,), (50,), (50,), (50, 2)] and all(a.rate == 16000 for a in got)
    for audio, (_, _, samples) in zip(got, cases.values()):
        assert np.array_equal(audio.data, samples)
    try:
        from scipy.io import wavfile
    except ImportError:
        return
    for name, audio in zip(cases, got):
        rate, data = wavfile.read(str(tmp_path / name))
        assert rate == audio.rate and data.dtype == audio.data.dtype and np.array_equal(data, audio.data), name


def test_reader_refusals(tmp_path, monkeypatch):
    from neuralmonkey_amd.readers.audio_reader import audio_reader
    with pytest.raises(ValueError, match="Unsupported audio format: mp3"):
        audio_reader(audio_format="mp3")
    write_wav(tmp_path / "i24.wav", 3, 1, 8000, np.zeros(30, np.uint8))
    (tmp_path / "noise.wav").write_bytes(b"not a wave file at all")
    (tmp_path / "files.list").write_text("i24.wav\n")
    with pytest.raises(ValueError, match="24-bit PCM is not supported"):
        list(audio_reader(str(tmp_path))([str(tmp_path / "files.list")]))
    (tmp_path / "files.list").write_text("noise.wav\n")
    with pytest.raises(ValueError, match="not a RIFF/WAVE PCM file"):
        list(audio_reader(str(tmp_path))([str(tmp_path / "files.list")]))
    # NIST Sphere files go through sph2pipe: without it on the PATH the reader says so
    empty = tmp_path / "bin"
    empty.mkdir()
    monkeypatch.setenv("PATH", str(empty))
    (tmp_path / "files.list").write_text("utterance.sph\n")
    with pytest.raises(RuntimeError, match="sph2pipe was not found on the PATH; it is needed to read .*utterance.sph"):
        list(audio_reader(str(tmp_path), audio_format="sph")([str(tmp_path / "files.list")]))
    # ... and its failure is the reference's RuntimeError
    tool = empty / "sph2pipe"
    tool.write_text("#!/bin/sh\nexit 3\n")
    tool.chmod(0o755)
    with pytest.raises(RuntimeError, match="sph2pipe exited with error code 3 when processing .*utterance.sph"):
        list(audio_reader(str(tmp_path), audio_format="sph")([str(tmp_path / "files.list")]))


# ---- the preprocessor -------------------------------------------------------------------------------------------------------
def test_preprocessor_refusals_fire_before_any_launch():
    """None of these reaches the device: there is none on this machine."""
    from neuralmonkey_amd.processors.speech import SpeechFeaturesPreprocessor as Pre
    from neuralmonkey_amd.readers.audio_reader import Audio
    with pytest.raises(ValueError, match="Unknown speech feature type 'plp'"):
        Pre("plp")
    for kind in ("fbank", "logfbank", "ssc"):
        for key, value in (("numcep", 13), ("ceplifter", 22), ("appendEnergy", True)):
            with pytest.raises(TypeError, match="unexpected keyword argument '{}'".format(key)):
                Pre(kind, **{key: value})
    with pytest.raises(TypeError, match="unexpected keyword argument 'samplerate'"):
        Pre("mfcc", samplerate=8000)
    for nfft in (32, 8192, 300, 0, 512.0):
        with pytest.raises(ValueError, match="nfft must be a power of two in 64..4096"):
            Pre("mfcc", nfft=nfft)
    with pytest.raises(ValueError, match="numcep must be in 1..nfilt = 26, not 27"):
        Pre("mfcc", numcep=27)
    with pytest.raises(ValueError, match="nfilt must be in 1..256"):
        Pre("fbank", nfilt=257)
    for window in (0, -1):
        with pytest.raises(ValueError, match="delta_window must be an integer in 1..64"):
            Pre("mfcc", 1, window)
    with pytest.raises(ValueError, match="delta_order -1 is negative"):
        Pre("mfcc", -1)
    with pytest.raises(TypeError, match="winfunc must be a callable"):
        Pre("mfcc", winfunc=3)
    mono = Audio(8000, np.zeros(100, np.int16))
    with pytest.raises(ValueError, match="highfreq is greater than samplerate/2"):
        Pre("mfcc", highfreq=4001)(mono)
    with pytest.raises(ValueError, match="highfreq is greater than samplerate/2"):
        Pre("ssc", highfreq=4001).many([mono, mono])
    with pytest.raises(ValueError, match=r"one channel: the audio data have shape \(100, 2\)"):
        Pre("mfcc")(Audio(8000, np.zeros((100, 2), np.int16)))
    with pytest.raises(ValueError, match="needs nfft = 8192"):
        Pre("mfcc")(Audio(192000, np.zeros(100, np.int16)))
    with pytest.raises(ValueError, match="returned an array of shape"):
        Pre("mfcc", winfunc=lambda n: np.ones(n + 1))(mono)


def test_tables_and_framing():
    from neuralmonkey_amd.processors.speech import SpeechFeaturesPreprocessor as Pre, frame_count
    pre = Pre("mfcc", 2)
    assert [(t.frame_len, t.frame_step, t.nfft) for t in map(pre.tables, (44100, 16000, 8000))] == [
        (1103, 441, 2048), (400, 160, 512), (200, 80, 256)]
    assert [speech_ref.framing(rate) for rate in (44100, 16000, 8000)] == [(1103, 441, 2048), (400, 160, 512),
                                                                           (200, 80, 256)]
    assert pre.tables(8000) is pre.tables(8000)                      # cached per rate on the object
    assert pre.num_features() == 39 and Pre("fbank", 1, nfilt=40).num_features() == 80
    for samples, want in ((0, 1), (50, 1), (200, 1), (201, 2), (280, 2), (281, 3), (50400, 629)):
        assert frame_count(samples, 200, 80) == speech_ref.num_frames(samples, 200, 80) == want
    tab = pre.tables(16000)
    assert tab.window.dtype == np.float32 and np.array_equal(tab.window, np.ones(400, np.float32))
    bank = speech_ref.filterbank(26, 512, 16000, 0, None)
    assert np.array_equal(tab.bank, bank.astype(np.float32)) and tab.bank.shape == (26, 257)
    for j, (first, last) in enumerate(tab.bank_range):
        assert 0 <= first < last <= 257 and not tab.bank[j, :first].any() and not tab.bank[j, last:].any()
        assert tab.bank[j, first] != 0 and tab.bank[j, last - 1] != 0
    lifter = 1 + 11 * np.sin(np.pi * np.arange(13) / 22)
    assert tab.dct.dtype == np.float32 and np.allclose(tab.dct, speech_ref.dct_matrix(13, 26) * lifter[:, None],
                                                       rtol=2e-7, atol=1e-8)
    k = np.arange(256)
    assert np.allclose(tab.twiddles[:, 0] + 1j * tab.twiddles[:, 1], np.exp(-2j * np.pi * k / 512), atol=1e-7)
    with pytest.warns(UserWarning, match=r"frame length \(400\) is greater than FFT size \(256\)"):
        assert Pre("mfcc", nfft=256).tables(16000).nfft == 256
    assert np.allclose(Pre("fbank", winfunc=np.hamming).tables(8000).window, np.hamming(200))
    assert Pre("ssc").tables(8000).centroid_freqs.shape == (129,) and tab.centroid_freqs is None
    try:
        from scipy.fftpack import dct
    except ImportError:
        return
    x = np.random.RandomState(0).randn(5, 26)
    assert np.allclose(dct(x, type=2, axis=1, norm="ortho")[:, :13], x @ speech_ref.dct_matrix(13, 26).T, atol=1e-12)


def test_restatement_on_two_committed_recordings(audio_root):
    from neuralmonkey_amd.readers.audio_reader import read_wav
    dtmf = read_wav(os.path.join(audio_root, "tests/data/dtmf/1.wav"))
    feats = speech_ref.features(dtmf.data, dtmf.rate, "mfcc", delta_order=1)
    assert feats.shape == (42, 26) and feats.dtype == np.float64 and np.isfinite(feats).all()
    assert speech_ref.mfcc(dtmf.data, dtmf.rate).shape == (42, 13)
    yesno = read_wav(os.path.join(audio_root, YESNO))
    assert speech_ref.features(yesno.data, yesno.rate, "mfcc", delta_order=2).shape == (629, 39)
    # deltas of a ramp are its slope away from the clamped edges, and 0 for a single frame
    ramp = np.arange(10, dtype=np.float64)[:, None] * np.array([[1.0, -2.0]])
    assert np.allclose(speech_ref.delta(ramp, 2)[2:-2], [[1.0, -2.0]]) and not speech_ref.delta(ramp[:1], 3).any()
    # an all-zero utterance sits in the eps branch everywhere
    silent = speech_ref.features(np.zeros(300, np.int16), 8000, "logfbank")
    assert silent.shape == (3, 26) and np.all(silent == np.log(2.0 ** -52))


# ---- dataset.load ---------------------------------------------------------------------------------------------------------
def test_load_hands_a_series_to_many_in_chunks_and_keeps_order_and_laziness(tmp_path, monkeypatch):
    from neuralmonkey_amd import dataset
    (tmp_path / "numbers.txt").write_text("".join("{}\n".format(i) for i in range(11)))
    read = []

    def reader(files):
        for path in files:
            for line in open(path):
                read.append(int(line))
                yield int(line)

    class Chunked:
        calls = []

        def __call__(self, item):
            raise AssertionError("many() is the route of a preprocessor that has one")

        def many(self, items):
            self.calls.append(list(items))
            return [item * 10 for item in items]
    monkeypatch.setattr(dataset, "MANY_ITEMS", 4)
    data = [(str(tmp_path / "numbers.txt"), reader), (Chunked(), "n")]
    eager = dataset.load("d", ["n", "tens"], data, dataset.BatchingScheme(batch_size=3))
    assert list(eager.get_series("tens")) == [i * 10 for i in range(11)]
    assert Chunked.calls == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10]]
    del Chunked.calls[:], read[:]
    lazy = dataset.load("d", ["n", "tens"], data, dataset.BatchingScheme(batch_size=3), buffer_size=4)
    assert not read and not Chunked.calls                              # nothing is read until somebody iterates
    tens = lazy.get_series("tens")
    assert next(tens) == 0 and Chunked.calls == [[0, 1, 2, 3]] and read == [0, 1, 2, 3]
    assert list(tens) == [i * 10 for i in range(1, 11)]
    # a plain callable is called item by item, as before
    plain = dataset.load("d", ["n", "neg"], [data[0], (lambda item: -item, "n")], dataset.BatchingScheme(batch_size=3))
    assert list(plain.get_series("neg")) == [-i for i in range(11)]


# ---- the archive ----------------------------------------------------------------------------------------------------------
def test_archive_members_are_data_and_settings_only(audio_root):
    with tarfile.open(BUNDLE) as tar:
        names = [m.name for m in tar.getmembers()]
    dtmf = ["{}.wav".format(i) for i in range(1, 10)] + ["test_2.wav", "test_3.wav", "test_6.wav", "labels.vocab",
                                                           "train.labels", "train.sound", "val.labels", "val.sound"]
    yesno = ["train.txt", "test.txt", "train.wavlist", "test.wavlist", "yesno.vocab"]
    assert sorted(names) == sorted(["tests/ctc.ini", "tests/audio-classifier.ini"]
                                   + ["tests/data/dtmf/" + n for n in dtmf] + ["tests/data/yesno/" + n for n in yesno]
                                   + ["tests/data/yesno/waves_yesno/{}.wav".format(n) for n in YESNO_KEPT])
    assert not [n for n in names if n.endswith((".py", ".sh"))]
    assert os.path.getsize(BUNDLE) < 1 << 20
    with open(os.path.join(audio_root, "tests/data/yesno/train.wavlist")) as handle:
        assert [line.strip() for _, line in zip(range(4), handle)] == ["waves_yesno/{}.wav".format(n)
                                                                         for n in YESNO_KEPT[:4]]
    with open(os.path.join(audio_root, "tests/data/yesno/test.wavlist")) as handle:
        assert [line.strip() for _, line in zip(range(2), handle)] == ["waves_yesno/{}.wav".format(n)
                                                                         for n in YESNO_KEPT[4:]]
    if os.path.isdir(REF):
        for rel in names:
            with open(os.path.join(REF, rel), "rb") as a, open(os.path.join(audio_root, rel), "rb") as b:
                assert a.read() == b.read(), rel


# ---- the binding table ------------------------------------------------------------------------------------------------------
def speech_header_symbols():
    text = open(os.path.join(ROOT, "include", "nmhip_speech.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(nm_[a-z0-9_]+)\s*\(", text))


@pytest.fixture(scope="module")
def lib():
    from neuralmonkey_amd import build
    build.build(verbose=False)
    from neuralmonkey_amd import _lib
    return _lib.load()


def test_speech_header_matches_its_binding_table(lib):
    from neuralmonkey_amd import _lib
    from .test_abi import header_symbols
    mine = speech_header_symbols()
    assert mine == set(_lib.SPEECH_SIGNATURES) == {"nm_speech_frames", "nm_speech_deltas"}
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith("SIGNATURES") and n != "SPEECH_SIGNATURES"]
    assert len(others) >= 13 and all(not mine & set(table) for table in others)
    assert not mine & header_symbols()
    for name, (res, args) in _lib.SPEECH_SIGNATURES.items():
        fn = getattr(lib, name)                                          # exported, and bound by load()
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_speech_entry_points_refuse_before_any_launch(lib):
    """Host buffers and a null stream: a call that got as far as a launch would fault or fail differently."""
    f32 = lambda n: (ctypes.c_float * n)()
    wav, window, tw, bank, dct, freqs, out = f32(1000), f32(200), f32(256), f32(26 * 129), f32(13 * 26), f32(129), f32(4096)
    soff, foff, ranges = (ctypes.c_int64 * 3)(0, 500, 1000), (ctypes.c_int64 * 3)(0, 5, 10), (ctypes.c_int32 * 52)()

    def frames(wav_=wav, soff_=soff, foff_=foff, u=2, ns=1000, nf=10, fl=200, fs=80, nfft=256, window_=window, tw_=tw,
               bank_=bank, ranges_=ranges, nfilt=26, dct_=dct, numcep=13, freqs_=freqs, mode=0, out_=out, ld=13):
        return lib.nm_speech_frames(None, wav_, soff_, foff_, u, ns, nf, fl, fs, nfft, 0.97, window_, tw_, bank_, ranges_,
                                    nfilt, dct_, numcep, freqs_, mode, 1, out_, ld)
    null = b"nm_speech_frames: null pointer"
    for kwargs, text in ((dict(wav_=None), null), (dict(soff_=None), null), (dict(foff_=None), null),
                         (dict(window_=None), null), (dict(tw_=None), null), (dict(bank_=None), null),
                         (dict(ranges_=None), null), (dict(out_=None), null),
                         (dict(dct_=None), b"nm_speech_frames: null dct in MFCC mode"),
                         (dict(freqs_=None, mode=3, ld=26), b"nm_speech_frames: null R in SSC mode"),
                         (dict(u=0), b"nm_speech_frames: U = 0 utterances"),
                         (dict(ns=-1), b"nm_speech_frames: total_samples -1"),
                         (dict(nf=-1), b"nm_speech_frames: total_frames -1 outside"),
                         (dict(nf=1 << 31), b"nm_speech_frames: total_frames 2147483648 outside"),
                         (dict(fl=0), b"nm_speech_frames: frame length 0 and step 80"),
                         (dict(fs=0), b"nm_speech_frames: frame length 200 and step 0"),
                         (dict(nfft=32), b"nm_speech_frames: nfft 32 is not a power of two in 64..4096"),
                         (dict(nfft=8192), b"nm_speech_frames: nfft 8192 is not a power of two"),
                         (dict(nfft=300), b"nm_speech_frames: nfft 300 is not a power of two"),
                         (dict(nfilt=0), b"nm_speech_frames: nfilt 0 outside 1..256"),
                         (dict(nfilt=257), b"nm_speech_frames: nfilt 257 outside 1..256"),
                         (dict(mode=4), b"nm_speech_frames: unknown mode 4"),
                         (dict(mode=-1), b"nm_speech_frames: unknown mode -1"),
                         (dict(numcep=0), b"nm_speech_frames: numcep 0 outside 1..nfilt = 26"),
                         (dict(numcep=27, ld=27), b"nm_speech_frames: numcep 27 outside 1..nfilt = 26"),
                         (dict(ld=12), b"nm_speech_frames: ld 12 below the block's width 13"),
                         (dict(mode=1, ld=25), b"nm_speech_frames: ld 25 below the block's width 26")):
        assert frames(**kwargs) < 0 and text in lib.nm_last_error(), (kwargs, lib.nm_last_error())
    assert frames(nf=0, wav_=None, out_=None, window_=None) == 0          # no frames: a no-op

    def deltas(out_=out, ld=39, foff_=foff, u=2, nf=10, width=13, order=0, window_=2):
        return lib.nm_speech_deltas(None, out_, ld, foff_, u, nf, width, order, window_)
    for kwargs, text in ((dict(out_=None), b"nm_speech_deltas: null pointer"),
                         (dict(foff_=None), b"nm_speech_deltas: null pointer"),
                         (dict(u=0), b"nm_speech_deltas: U = 0 utterances"),
                         (dict(nf=-1), b"nm_speech_deltas: total_frames -1 outside"),
                         (dict(nf=1 << 31), b"nm_speech_deltas: total_frames 2147483648 outside"),
                         (dict(width=0), b"nm_speech_deltas: block width F 0 outside"),
                         (dict(order=-1), b"nm_speech_deltas: order -1 outside"),
                         (dict(window_=0), b"nm_speech_deltas: window N 0 outside 1..64"),
                         (dict(window_=65), b"nm_speech_deltas: window N 65 outside 1..64"),
                         (dict(order=2), b"nm_speech_deltas: ld 39 below (order + 2) * F = 52"),
                         (dict(ld=25), b"nm_speech_deltas: ld 25 below (order + 2) * F = 26")):
        assert deltas(**kwargs) < 0 and text in lib.nm_last_error(), (kwargs, lib.nm_last_error())
    assert deltas(nf=0, out_=None) == 0


def test_kernels_of_the_speech_file_do_not_spill(lib):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from kernel_resources import kernel_resources
    finally:
        sys.path.pop(0)
    mine = {k: v for k, v in kernel_resources().items() if "speech_frames_kernel" in k or "speech_deltas_kernel" in k}
    assert len(mine) == 2, sorted(mine)
    assert all(v["scratch"] == 0 and v["lds"] == 0 and v["max_threads"] == 256 for v in mine.values())
