"""``LogitsRunner``: a classifier's logits, or the distribution over its classes, written out as text (interface of
neuralmonkey/runners/logits_runner.py:15-105).

Per sentence the runner returns a list holding ONE string: for every decoding step (a Classifier has one) the values of
that step joined by commas, the steps joined by tabs.  Three things the reference does are kept because configurations
and downstream scripts see them (:43-49): with ``normalize`` the values are exp(x) / sum(exp(x)) computed on the host
without the row maximum subtracted, so logits beyond float32's exp range come out as nan; ``pick_index`` is tested for
truth, so index 0 behaves like None and every class is written; and exactly one session's result is accepted (:27-29).
[B, K] floats per step cross to the host, which is what the runner is for."""
from typing import Any, Dict, List, Optional

import numpy as np

from ..checking import check_argument_types
from ..decoders.classifier import Classifier
from .base_runner import BaseRunner


def format_step(values: np.ndarray, normalize: bool, pick_index: Optional[int]) -> str:
    """One sentence's values of one decoding step as text."""
    values = np.asarray(values)
    if normalize:
        weights = np.exp(values)                 # (no maximum subtracted: see the module docstring)
        values = weights / weights.sum(axis=0)
    if pick_index:                               # (0 counts as "no index")
        return str(values[pick_index])
    return ",".join(map(str, values))


class LogitsRunner(BaseRunner):
    """Writes ``decoder.decoded_logits`` [T, B, K] as one tab / comma separated string per sentence."""

    class Executable(BaseRunner.Executable):
        def collect_results(self, results: List[Dict]) -> None:
            if len(results) != 1:
                raise ValueError("LogitsRunner needs exactly 1 execution result, got {}".format(len(results)))
            fetched, runner = results[0], self.executor
            steps = np.asarray(fetched["logits"])                          # [T, B, K]
            sentences = [["\t".join(format_step(step[b], runner.normalize, runner.pick_index) for step in steps)]
                         for b in range(steps.shape[1])]
            self.set_runner_result(outputs=sentences, losses=[fetched["train_loss"], fetched["runtime_loss"]])

    def __init__(self,
                 output_series: str,
                 decoder: Classifier,
                 normalize: bool = True,
                 pick_index: int = None,
                 pick_value: str = None) -> None:
        """``normalize``: softmax the logits on the host.  ``pick_index`` / ``pick_value`` (at most one of the two):
        write a single class, named by its index or by its word in the decoder's vocabulary."""
        check_argument_types()
        BaseRunner.__init__(self, output_series, decoder)
        if pick_index is not None and pick_value is not None:
            raise ValueError("Either a pick index or a vocabulary value can be specified, not both at the same time.")
        if pick_value is not None:
            if pick_value not in decoder.vocabulary:
                raise ValueError("Value '{}' is not in vocabulary of decoder '{}'".format(pick_value, decoder.name))
            pick_index = decoder.vocabulary.index_to_word.index(pick_value)
        self.normalize = normalize
        self.pick_index: Optional[int] = pick_index

    @property
    def fetches(self) -> Dict[str, Any]:
        dec = self.decoder
        return {"logits": dec.decoded_logits, "train_loss": dec.train_loss, "runtime_loss": dec.runtime_loss}

    @property
    def loss_names(self) -> List[str]:
        return ["train_loss", "runtime_loss"]
