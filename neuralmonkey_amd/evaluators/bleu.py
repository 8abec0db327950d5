"""BLEU with the smoothing of mteval-v13a (the interface and the numbers of neuralmonkey/evaluators/bleu.py).

One thing to know before reading a score.  The "true positives" of an order are NOT a clipped count: they are the
number of reference windows whose n-gram occurs in the hypothesis at least once (bleu.py:122-124 adds the reference's
count over the distinct hypothesis n-grams), so a hypothesis "a a" against "a a a a a a" earns 6 unigrams for the 2 it
produced.  The sentence-level rewards of ``ReinforceObjective`` are these numbers, and csrc/nm_rl.hip computes the same
on token indices, so the rule is kept as it is and lives in one place here: ``found_in_references``.
"""
from collections import Counter
from typing import Iterator, List, Tuple

import numpy as np

from ..checking import check_argument_types
from .evaluator import Evaluator


def _windows(words: List[str], order: int, fold_case: bool, glue: str) -> Iterator[str]:
    """The n-grams of ``words`` as glued strings, in order of their start."""
    for start in range(len(words) - order + 1):
        gram = glue.join(words[start:start + order])
        yield gram.lower() if fold_case else gram


def found_in_references(hypothesis: List[str], references: List[List[str]], order: int,
                        fold_case: bool) -> Tuple[int, int, int]:
    """For one sentence and one order: (reference windows whose n-gram the hypothesis holds, hypothesis windows,
    reference windows).  Several references count an n-gram as often as the one that holds it most often."""
    budget = BLEUEvaluator.merge_max_counters([BLEUEvaluator.ngram_counts(ref, order, fold_case) for ref in references])
    produced = BLEUEvaluator.ngram_counts(hypothesis, order, fold_case)
    found = sum(times for gram, times in budget.items() if gram in produced)
    return found, sum(produced.values()), sum(budget.values())


class BLEUEvaluator(Evaluator):

    def __init__(self, n: int = 4, deduplicate: bool = False, name: str = None,
                 multiple_references_separator: str = None) -> None:
        """``n``: the longest n-grams counted.  ``deduplicate``: a token repeated in a row counts once in a hypothesis.
        ``multiple_references_separator``: the token that parts several references given as one sentence."""
        check_argument_types()
        if name is None:
            name = "BLEU-{}{}".format(n, "-dedup" if deduplicate else "")
        super().__init__(name)
        self.n = n
        self.deduplicate = deduplicate
        self.multiple_references_separator = multiple_references_separator

    def _reference_groups(self, references: List[List[str]]) -> List[List[List[str]]]:
        mark = self.multiple_references_separator
        if mark is None:
            return [[sentence] for sentence in references]
        grouped = []
        for sentence in references:
            parts = [[]]            # type: List[List[str]]
            for token in sentence:
                if token == mark:
                    parts.append([])
                else:
                    parts[-1].append(token)
            grouped.append(parts)
        return grouped

    def score_batch(self, hypotheses: List[List[str]], references: List[List[str]]) -> float:
        if self.deduplicate:
            hypotheses = self.deduplicate_sentences(hypotheses)
        return 100 * self.bleu(hypotheses, self._reference_groups(references), self.n)

    # -- counting -------------------------------------------------------------------------------------------------
    @staticmethod
    def ngram_counts(sentence: List[str], n: int, lowercase: bool, delimiter: str = " ") -> Counter:
        """How often each n-gram (its words glued by ``delimiter``) occurs in ``sentence``."""
        return Counter(_windows(sentence, n, lowercase, delimiter))

    @staticmethod
    def merge_max_counters(counters: List[Counter]) -> Counter:
        """Per key the largest count any of ``counters`` holds."""
        top = Counter()  # type: Counter
        for counts in counters:
            top |= counts                                    # Counter union keeps the maximum
        return top

    @staticmethod
    def modified_ngram_precision(hypotheses: List[List[str]], references_list: List[List[List[str]]], n: int,
                                 case_sensitive: bool) -> Tuple[float, int]:
        """(precision of order ``n`` over the corpus, hypothesis n-grams in the corpus); a corpus without such an
        n-gram has precision 1."""
        found = produced = 0
        for hypothesis, references in zip(hypotheses, references_list):
            hits, made, _ = found_in_references(hypothesis, references, n, not case_sensitive)
            found, produced = found + hits, produced + made
        return (found / produced, produced) if produced else (1, 0)

    # -- lengths ----------------------------------------------------------------------------------------------------
    @staticmethod
    def effective_reference_length(hypotheses: List[List[str]], references_list: List[List[List[str]]]) -> int:
        """Per sentence the length of the reference closest in length to the hypothesis (the first of several), summed."""
        total = 0
        for hypothesis, references in zip(hypotheses, references_list):
            if references:
                total += len(min(references, key=lambda ref, size=len(hypothesis): abs(len(ref) - size)))
        return total

    @staticmethod
    def minimum_reference_length(hypotheses: List[List[str]],                    # pylint: disable=unused-argument
                                 references_list: List[List[str]]) -> int:
        """Per sentence the length of its shortest reference, summed."""
        return sum(min((len(ref) for ref in references), default=np.inf) for references in references_list)

    # -- the score ----------------------------------------------------------------------------------------------------
    @staticmethod
    def bleu(hypotheses: List[List[str]], references: List[List[List[str]]], ngrams: int = 4,
             case_sensitive: bool = True):
        """exp(mean over the orders of log precision + brevity term), between 0 and 1.  An order without a single match
        takes 1 / (2^k * its hypothesis n-grams) for its precision, k counting such orders so far: mteval-v13a."""
        share = 1 / ngrams
        log_score, halvings = 0, 1.0
        for order in range(1, ngrams + 1):
            precision, produced = BLEUEvaluator.modified_ngram_precision(hypotheses, references, order, case_sensitive)
            if precision == 0:
                halvings *= 2
                precision = 1 / (halvings * produced)
            log_score += share * np.log(precision)
        reference_words = BLEUEvaluator.effective_reference_length(hypotheses, references)
        hypothesis_words = sum(len(sentence) for sentence in hypotheses)
        if hypothesis_words == 0:
            brevity = -np.inf
        else:
            brevity = min(1 - reference_words / hypothesis_words, 0)
        return np.exp(log_score + brevity)

    @staticmethod
    def deduplicate_sentences(sentences: List[List[str]]) -> List[List[str]]:
        """Every run of one repeated token shrinks to a single token."""
        return [[word for at, word in enumerate(sentence) if at == 0 or word != sentence[at - 1]]
                for sentence in sentences]
