"""MBRRunner: the sample an ``MBRDecoder`` chose for every sentence as an output series (the reference has no
counterpart; the shape is ``SamplingRunner``'s with the decoder's choice where that has a fixed sample index).

The output is the chosen sample cut at </s>; the loss ``expected_utility`` is the batch mean of the chosen samples'
expected utilities, ``expected[b, best[b]]``."""
from typing import TYPE_CHECKING, Any, Callable, Dict, List

import numpy as np

from .base_runner import BaseRunner, NextExecute

if TYPE_CHECKING:                                         # decoders/mbr_decoder.py imports trainers/, which imports runners/
    from ..decoders.mbr_decoder import MBRDecoder       # noqa: F401  pylint: disable=cyclic-import


class MBRRunner(BaseRunner):
    class Executable(BaseRunner.Executable):
        def __init__(self, executor: "MBRRunner", compute_losses: bool, summaries: bool, num_sessions: int) -> None:
            super().__init__(executor, compute_losses, summaries, num_sessions)
            if num_sessions > 1:
                raise NotImplementedError("MBRRunner: sampling from an ensemble ({} sessions) is not implemented"
                                          .format(num_sessions))
            self.decoder = executor.decoder
            self.postprocess = executor.postprocess

        def next_to_execute(self) -> NextExecute:
            return {"mbr": self.decoder.outputs}, [{}]

        def collect_results(self, results: List[Dict]) -> None:
            self.prepare_results(results[0]["mbr"])

        def prepare_results(self, output) -> None:
            tok_tb = np.asarray(output.token_ids)
            if tok_tb.shape[0] == 0:
                decoded_tokens = [[] for _ in range(tok_tb.shape[1])]
            else:
                decoded_tokens = self.decoder.vocabulary.vectors_to_sentences(tok_tb)
            if self.postprocess is not None:
                decoded_tokens = self.postprocess(decoded_tokens)
            best = np.asarray(output.best)
            expected = np.asarray(output.expected_utility)[np.arange(best.shape[0]), best]
            self.set_runner_result(outputs=decoded_tokens, losses=[float(np.mean(expected))])

    def __init__(self, output_series: str, decoder: "MBRDecoder",
                 postprocess: Callable[[List[str]], List[str]] = None) -> None:
        super().__init__(output_series, decoder)
        self.postprocess = postprocess

    def ahead_fetches(self) -> List[Any]:
        from .base_runner import encoder_side_fetches
        return encoder_side_fetches(self.decoder.sampling_decoder.parent_decoder)

    @property
    def fetches(self) -> Dict[str, Any]:
        return {"mbr": self.decoder.outputs}

    @property
    def loss_names(self) -> List[str]:
        return ["expected_utility"]
