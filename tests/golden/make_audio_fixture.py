"""The fixtures of the speech front end's tests, made where the reference tree is:

    python tests/golden/make_audio_fixture.py

* tests/golden/reference_tests_audio.tar.gz -- tests/ctc.ini and tests/audio-classifier.ini, tests/data/dtmf in full and
  tests/data/yesno (texts, vocabulary, list files and recordings), the reference's bytes, bundled the way
  make_reference_ini_fixture.py bundles its archives: configurations and data only, no program text.  All 15 yesno
  recordings go in if the archive then stays under the limit for a committed file; otherwise only those named by the
  first ``TRAIN_LINES`` lines of train.wavlist and the first ``TEST_LINES`` of test.wavlist (the test shortens the
  lists it uses to match);
* tests/golden/speech_signatures.json -- the parameters of ``audio_reader`` and ``SpeechFeaturesPreprocessor``, read from
  the reference's source as tests/test_reference_signatures.py reads them."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from make_reference_ini_fixture import REF, members, write  # noqa: E402  pylint: disable=wrong-import-position

OUT = os.path.join(HERE, "reference_tests_audio.tar.gz")
OUT_SIGNATURES = os.path.join(HERE, "speech_signatures.json")
LIMIT = 1 << 20
TRAIN_LINES, TEST_LINES = 4, 2
SIGNATURES = [("readers/audio_reader.py", "audio_reader"), ("processors/speech.py", "SpeechFeaturesPreprocessor")]
YESNO_TEXT = ["yesno/train.txt", "yesno/test.txt", "yesno/train.wavlist", "yesno/test.wavlist", "yesno/yesno.vocab"]


def listed(name, count):
    with open(os.path.join(REF, "tests/data/yesno", name)) as handle:
        return ["yesno/" + line.rstrip() for _, line in zip(range(count), handle)]


def main():
    base = ["dtmf/*"] + YESNO_TEXT
    write(OUT, members(["ctc", "audio-classifier"], base + ["yesno/waves_yesno/*.wav"]))
    if os.path.getsize(OUT) >= LIMIT:
        write(OUT, members(["ctc", "audio-classifier"],
                           base + listed("train.wavlist", TRAIN_LINES) + listed("test.wavlist", TEST_LINES)))
    assert os.path.getsize(OUT) < LIMIT
    from tests.test_reference_signatures import read_reference_parameters
    found = {}
    for path, name in SIGNATURES:
        found.setdefault(path, {})[name] = read_reference_parameters(path, name)
    with open(OUT_SIGNATURES, "w", encoding="utf-8") as handle:
        json.dump(found, handle, indent=1)
        handle.write("\n")
    print(OUT_SIGNATURES)


if __name__ == "__main__":
    main()
