"""Series reader for audio files (interface of neuralmonkey/readers/audio_reader.py): a dataset series given as
``(list files, audio_reader(prefix))`` yields one ``Audio(rate, data)`` per line of the list files.  Host side only --
the samples reach the device through ``processors.speech.SpeechFeaturesPreprocessor``.

RIFF/WAVE PCM is read with the standard library's ``wave`` and NumPy, with the dtypes ``scipy.io.wavfile.read`` (the
reference's reader) returns: 8-bit ``uint8``, 16-bit ``int16``, 32-bit ``int32``; one channel comes back as ``[n]``,
several as ``[n, channels]``.  Other sample widths (24-bit PCM, which scipy widens to int32) and non-PCM encodings are
refused with a ValueError that names the file.  NIST Sphere files (``audio_format="sph"``) are converted to WAV by the
external ``sph2pipe`` tool, as in the reference, and then read the same way."""
import io
import os
import subprocess
import wave
from typing import Callable, Iterator, List, NamedTuple

import numpy as np

PCM_DTYPES = {1: np.dtype("uint8"), 2: np.dtype("<i2"), 4: np.dtype("<i4")}


class Audio(NamedTuple):
    """One recording: ``rate`` in samples per second and ``data``, the integer PCM samples as they are in the file
    (``[n]``, or ``[n, channels]`` for more than one channel)."""
    rate: int
    data: np.ndarray


def read_wav(source, what: str = None) -> Audio:
    """``Audio(rate, samples)`` of a RIFF/WAVE PCM file (a path or a binary file object)."""
    what = what if what is not None else str(source)
    try:
        with wave.open(source, "rb") as handle:
            rate, width, channels = handle.getframerate(), handle.getsampwidth(), handle.getnchannels()
            raw = handle.readframes(handle.getnframes())
    except wave.Error as exc:
        raise ValueError("{}: not a RIFF/WAVE PCM file ({})".format(what, exc)) from None
    if width not in PCM_DTYPES:
        raise ValueError("{}: {}-bit PCM is not supported (8, 16 or 32 bits)".format(what, 8 * width))
    data = np.frombuffer(raw, dtype=PCM_DTYPES[width])
    data = data.astype(data.dtype.newbyteorder("="))          # native byte order, and a writable copy
    if channels > 1:
        data = data[:len(data) // channels * channels].reshape(-1, channels)
    return Audio(rate, data)


def read_sph(path: str) -> Audio:
    """A NIST Sphere file, converted by ``sph2pipe -f wav`` (which writes the WAV file to its standard output)."""
    try:
        done = subprocess.run(["sph2pipe", "-f", "wav", path], stdout=subprocess.PIPE, check=False)
    except FileNotFoundError as exc:
        raise RuntimeError("sph2pipe was not found on the PATH; it is needed to read {}".format(path)) from exc
    if done.returncode != 0:              # (the reference's message)
        raise RuntimeError("sph2pipe exited with error code {} when processing {}".format(done.returncode, path))
    return read_wav(io.BytesIO(done.stdout), path)


FORMATS = {"wav": read_wav, "sph": read_sph}


def audio_reader(prefix: str = "", audio_format: str = "wav") -> Callable[[List[str]], Iterator[Audio]]:
    """A reader for a dataset series of recordings.  The reader takes list files; every line of a list file names one
    recording, relative to ``prefix``, in the format ``audio_format`` ("wav" or "sph"); it yields their ``Audio`` in the
    lines' order.  Any other format is refused here, before a file is opened."""
    if audio_format not in FORMATS:
        raise ValueError("Unsupported audio format: {}".format(audio_format))
    read_one = FORMATS[audio_format]

    def recordings(list_files: List[str]) -> Iterator[Audio]:
        for list_path in list_files:
            with open(list_path, encoding="utf-8") as names:
                for name in names:
                    yield read_one(os.path.join(prefix, name.rstrip()))
    return recordings
