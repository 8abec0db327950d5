"""SamplingRunner: the samples of a ``SamplingDecoder`` as output series (the reference has no counterpart; the shape is
``BeamSearchRunner``'s, runners/beamsearch_runner.py:84-106 and :154-190, with a sample index where that has a rank).

One runner emits sample ``sample`` (1 .. ``num_samples``) of every sentence, cut at </s>; its loss is the mean of
those samples' summed log-probabilities under the truncated distributions they were drawn from."""
from typing import Any, Callable, Dict, List

import numpy as np

from ..decoders.sampling_decoder import SamplingDecoder
from .base_runner import BaseRunner, NextExecute


class SamplingRunner(BaseRunner):
    class Executable(BaseRunner.Executable):
        def __init__(self, executor: "SamplingRunner", compute_losses: bool, summaries: bool,
                     num_sessions: int) -> None:
            super().__init__(executor, compute_losses, summaries, num_sessions)
            if num_sessions > 1:
                raise NotImplementedError("SamplingRunner: sampling from an ensemble ({} sessions) is not implemented"
                                          .format(num_sessions))
            self.sample = executor.sample
            self.decoder = executor.decoder
            self.postprocess = executor.postprocess

        def next_to_execute(self) -> NextExecute:
            return {"samples": self.decoder.outputs}, [{}]

        def collect_results(self, results: List[Dict]) -> None:
            self.prepare_results(results[0]["samples"])

        def prepare_results(self, output) -> None:
            tok_tb = np.asarray(output.token_ids)[:, :, self.sample - 1]
            if tok_tb.shape[0] == 0:
                decoded_tokens = [[] for _ in range(tok_tb.shape[1])]
            else:
                decoded_tokens = self.decoder.vocabulary.vectors_to_sentences(tok_tb)
            if self.postprocess is not None:
                decoded_tokens = self.postprocess(decoded_tokens)
            logprobs = np.asarray(output.logprob_sum)[:, self.sample - 1]
            self.set_runner_result(outputs=decoded_tokens, losses=[float(np.mean(logprobs))])

    def __init__(self, output_series: str, decoder: SamplingDecoder, sample: int = 1,
                 postprocess: Callable[[List[str]], List[str]] = None) -> None:
        super().__init__(output_series, decoder)
        if sample < 1 or sample > decoder.num_samples:
            raise ValueError("The index of the output sample must be between 1 and the number of samples ({}), "
                             "was {}.".format(decoder.num_samples, sample))
        self.sample = sample
        self.postprocess = postprocess

    def ahead_fetches(self) -> List[Any]:
        from .base_runner import encoder_side_fetches
        return encoder_side_fetches(self.decoder.parent_decoder)

    @property
    def fetches(self) -> Dict[str, Any]:
        return {"samples": self.decoder.outputs}

    @property
    def loss_names(self) -> List[str]:
        return ["sample_logprob"]


def sampling_runner_range(output_series: str, decoder: SamplingDecoder, max_sample: int = None,
                          postprocess: Callable[[List[str]], List[str]] = None) -> List[SamplingRunner]:
    """One runner per sample 1 .. ``max_sample`` (default: every sample the decoder draws)."""
    if max_sample is None:
        max_sample = decoder.num_samples
    if max_sample > decoder.num_samples:
        raise ValueError("The maximum sample index ({}) cannot be bigger than the number of samples {}."
                         .format(max_sample, decoder.num_samples))
    return [SamplingRunner("{}.sample{:03d}".format(output_series, s), decoder, s, postprocess)
            for s in range(1, max_sample + 1)]
