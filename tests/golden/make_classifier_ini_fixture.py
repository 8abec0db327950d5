"""Bundle the reference's sentence-classification and regression configs and the data files they name that no committed
archive holds yet into tests/golden/reference_tests_classifier.tar.gz, the way make_reference_ini_fixture.py makes its
archives (the members are the reference's bytes, nothing is edited; configs and data only -- no reference source code).

    python tests/golden/make_classifier_ini_fixture.py        (where the reference tree is)

tests/classifier.ini: a SentenceEncoder read by an AttentiveEncoder and a SequenceMaxPooling (and a SequenceCNNEncoder,
which this engine does not ship), two Classifiers -- one through a gradient-reversal StatefulView -- GreedyRunner and
LogitsRunner.  tests/regressor.ini: a SentenceEncoder under a SequenceRegressor and a RegressionRunner.  The parallel
text and the encoder vocabulary they also name are in reference_tests.tar.gz."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_reference_ini_fixture import members, write  # noqa: E402  pylint: disable=wrong-import-position

OUT_CLASSIFIER = os.path.join(HERE, "reference_tests_classifier.tar.gz")
INIS_CLASSIFIER = ["classifier", "regressor"]
DATA_CLASSIFIER = ["train.words", "val.words", "classification.vocab", "train.tc.counts", "val.tc.counts"]


if __name__ == "__main__":
    write(OUT_CLASSIFIER, members(INIS_CLASSIFIER, DATA_CLASSIFIER))
