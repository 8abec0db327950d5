"""Bundle the reference's language-model config and the word2vec sample it names into
tests/golden/reference_tests_language_model.tar.gz, the way make_reference_ini_fixture.py makes its archives (the members
are the reference's bytes, nothing is edited; a config and a data file only -- no reference source code).

    python tests/golden/make_language_model_ini_fixture.py        (where the reference tree is)

tests/language-model.ini: a Decoder without encoders whose vocabulary and embedding matrix come from
tests/data/sample.w2v (util.word2vec), trained by a CrossEntropyTrainer and scored by an XentRunner.  The corpora it names
are in reference_tests.tar.gz."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_reference_ini_fixture import members, write  # noqa: E402  pylint: disable=wrong-import-position

OUT_LANGUAGE_MODEL = os.path.join(HERE, "reference_tests_language_model.tar.gz")
INIS_LANGUAGE_MODEL = ["language-model"]
DATA_LANGUAGE_MODEL = ["sample.w2v"]


if __name__ == "__main__":
    write(OUT_LANGUAGE_MODEL, members(INIS_LANGUAGE_MODEL, DATA_LANGUAGE_MODEL))
