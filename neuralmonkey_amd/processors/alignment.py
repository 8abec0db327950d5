"""Word alignments in text form as fixed-shape matrices (mirror of neuralmonkey/processors/alignment.py:11-57; host
side, pure NumPy: the matrices are the labels WordAlignmentDecoder feeds to the device).

A sentence is a list of tokens ``s-t`` or ``s:t/w``: the index of a source word, the index of a target word and an
optional weight (1 when absent); ``-`` and ``:`` are interchangeable.  The result is ``[target_len, source_len]`` with
``result[t][s] = w``; pairs outside that shape are dropped; with ``normalize`` every row is divided by its sum and a row
without any aligned word (0 / 0) stays zero; ``zero_based=False`` reads indices that count from 1."""
import re
from typing import List

import numpy as np

ID_SEP = re.compile(r"[-:]")


# pylint: disable=too-few-public-methods
class WordAlignmentPreprocessor:
    def __init__(self, source_len, target_len, dtype=np.float32, normalize=True, zero_based=True):
        self._source_len = source_len
        self._target_len = target_len
        self._dtype = dtype
        self._normalize = normalize
        self._zero_based = zero_based

    def __call__(self, sentence: List[str]):
        result = np.zeros((self._target_len, self._source_len), self._dtype)
        shift = 0 if self._zero_based else 1
        for token in sentence:
            ids, _, weight = token.partition("/")
            src, tgt = (int(piece) - shift for piece in ID_SEP.split(ids))
            # (only the upper bounds are checked, as in the reference: a negative index counts from the end)
            if src < self._source_len and tgt < self._target_len:
                result[tgt][src] = float(weight) if weight else 1.
        if self._normalize:
            with np.errstate(divide="ignore", invalid="ignore"):
                result /= result.sum(axis=1, keepdims=True)
                result[np.isnan(result)] = 0
        return result
