"""Bundle the reference's two tagging configs and the data they name into tests/golden/reference_tests_labeler.tar.gz,
the way make_reference_ini_fixture.py makes its archives (the members are the reference's bytes, nothing is edited;
configs and data only -- no reference source code).

    python tests/golden/make_labeler_ini_fixture.py        (where the reference tree is)

tests/labeler.ini: POS tagging, a three-layer RecurrentEncoder under a SequenceLabeler.  tests/bert.ini: a masked
language model, TransformerEncoder + EmbeddingsLabeler + LabelRunner + XentRunner under DelayedUpdateTrainer."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_reference_ini_fixture import members, write  # noqa: E402  pylint: disable=wrong-import-position

OUT_LABELER = os.path.join(HERE, "reference_tests_labeler.tar.gz")
INIS_LABELER = ["labeler", "bert"]
DATA_LABELER = ["labeler/*", "bert/*", "factored_decoder_vocab.tsv", "factored_tag_vocab.tsv"]


if __name__ == "__main__":
    write(OUT_LABELER, members(INIS_LABELER, DATA_LABELER))
