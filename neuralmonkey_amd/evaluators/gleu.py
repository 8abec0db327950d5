"""GLEU (Wu et al. 2016, https://arxiv.org/abs/1609.08144): the smaller of precision and recall over all n-grams up to
``n`` together (the interface and the numbers of neuralmonkey/evaluators/gleu.py).  The counting is ``bleu.py``'s
``found_in_references``, with its unclipped true positives (gleu.py:80-82)."""
from typing import List, Tuple

from ..checking import check_argument_types
from .bleu import BLEUEvaluator, found_in_references
from .evaluator import Evaluator, check_lengths


class GLEUEvaluator(Evaluator):

    def __init__(self, n: int = 4, deduplicate: bool = False, name: str = None) -> None:
        check_argument_types()
        if name is None:
            name = "GLEU-{}{}".format(n, "-dedup" if deduplicate else "")
        super().__init__(name)
        self.n = n
        self.deduplicate = deduplicate

    @check_lengths
    def score_batch(self, hypotheses: List[List[str]], references: List[List[str]]) -> float:
        if self.deduplicate:
            hypotheses = BLEUEvaluator.deduplicate_sentences(hypotheses)
        return self.gleu(hypotheses, [[sentence] for sentence in references], self.n)

    @staticmethod
    def total_precision_recall(hypotheses: List[List[str]], references_list: List[List[List[str]]], ngrams: int,
                               case_sensitive: bool) -> Tuple[float, float]:
        """(precision, recall) with the counts of the orders 1 .. ``ngrams`` pooled.  (0, 0) once the orders so far
        have found no n-gram at all in the hypotheses."""
        found = produced = wanted = 0
        for order in range(1, ngrams + 1):
            for hypothesis, references in zip(hypotheses, references_list):
                hits, made, asked = found_in_references(hypothesis, references, order, not case_sensitive)
                found, produced, wanted = found + hits, produced + made, wanted + asked
            if produced == 0:
                return 0, 0
        return found / produced, found / wanted

    @staticmethod
    def gleu(hypotheses: List[List[str]], references: List[List[List[str]]], ngrams: int = 4,
             case_sensitive: bool = True) -> float:
        return min(GLEUEvaluator.total_precision_recall(hypotheses, references, ngrams, case_sensitive))
