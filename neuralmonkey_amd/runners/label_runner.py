"""``LabelRunner``: one label per input token from a SequenceLabeler (interface of
neuralmonkey/runners/label_runner.py:17-68).

The reference fetches the [B,T,K] log-probabilities and the input mask, takes the argmax on the host and overwrites
masked positions with END_TOKEN_INDEX (:34-39).  Here the labelling kernel does both on the device
(``decoder.labels``), so B*T int32 words cross to the host.  The argmax is taken over the logits, not over the
log-probabilities; the two can differ only where subtracting the row's log-sum-exp rounds two distinct logits to one
float -- an exact tie after rounding, which the first-maximum rule then breaks the same way unless the rounding
itself reorders them.

Several sessions (ensembles) are not supported: the reference's own loop over further session results compares two
arrays with a bare ``assert a == b`` (:32), which raises for any batch of more than one element, so there is no
behaviour to mirror."""
from typing import Any, Callable, Dict, List

import numpy as np

from ..checking import check_argument_types
from ..decoders.sequence_labeler import SequenceLabeler
from .base_runner import BaseRunner

Postprocessor = Callable[[List[List[str]]], List[List[str]]]


class LabelRunner(BaseRunner):
    class Executable(BaseRunner.Executable):
        def collect_results(self, results: List[Dict]) -> None:
            if len(results) != 1:
                raise ValueError("LabelRunner needs exactly 1 execution result, got {}".format(len(results)))
            (fetched,), runner = results, self.executor
            labels = np.asarray(fetched["labels"])                        # [B,T]; vectors_to_sentences is time-major
            sentences = runner.decoder.vocabulary.vectors_to_sentences(np.ascontiguousarray(labels.T))
            if runner.postprocess is not None:
                sentences = runner.postprocess(sentences)
            self.set_runner_result(outputs=sentences, losses=[float(fetched.get("loss", 0.0))])

    def __init__(self, output_series: str, decoder: SequenceLabeler, postprocess: Postprocessor = None) -> None:
        check_argument_types()
        BaseRunner.__init__(self, output_series, decoder)
        self.postprocess = postprocess

    @property
    def fetches(self) -> Dict[str, Any]:
        return {"labels": self.decoder.labels, "loss": self.decoder.cost}

    @property
    def loss_names(self) -> List[str]:
        return ["loss"]
