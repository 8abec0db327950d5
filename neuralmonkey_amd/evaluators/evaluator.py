"""What every evaluator has in common (the interface of neuralmonkey/evaluators/evaluator.py:12-119): a display name,
a score for one prediction, a score for a batch, and an order on scores."""
import functools
from typing import Any, List

import numpy as np

from ..checking import check_argument_types


def check_lengths(scorer):
    """Decorator of a ``score_batch``: both lists must be equally long and hold at least one pair."""
    @functools.wraps(scorer)
    def checked(self, hypotheses, references):
        pairs, wanted = len(hypotheses), len(references)
        if pairs != wanted:
            raise ValueError("Hypothesis and reference lists do not have the same length: {} vs {}.".format(pairs, wanted))
        if pairs == 0:
            raise ValueError("No hyp/ref pair to evaluate.")
        return scorer(self, hypotheses, references)
    return checked


class Evaluator:
    """Called with the predictions of a batch and their references, an evaluator answers with one number.  Subclasses
    override ``score_batch`` (corpus-level measures) or ``score_instance`` (whose mean the default batch score is)."""

    SUFFIX = "Evaluator"

    def __init__(self, name: str = None) -> None:
        check_argument_types()
        if name is None:                         # the class name without its suffix: "GLEUEvaluator" shows as "GLEU"
            own = type(self).__name__
            name = own[:-len(self.SUFFIX)] if own.endswith(self.SUFFIX) else own
        self._name = name

    name = property(lambda self: self._name)

    def score_instance(self, hypothesis: Any, reference: Any) -> float:      # pylint: disable=no-self-use
        """Exact match: 1.0 or 0.0."""
        return float(hypothesis == reference)

    @check_lengths
    def score_batch(self, hypotheses: List[Any], references: List[Any]) -> float:
        return np.mean([self.score_instance(*pair) for pair in zip(hypotheses, references)])

    def __call__(self, hypotheses: List[Any], references: List[Any]) -> float:
        return self.score_batch(hypotheses, references)

    @staticmethod
    def compare_scores(score1: float, score2: float) -> int:
        """The sign of ``score1 - score2``: bigger is better."""
        if score1 == score2:
            return 0
        return 1 if score1 > score2 else -1
