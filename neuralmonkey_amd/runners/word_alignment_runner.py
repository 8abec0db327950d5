"""``WordAlignmentRunner``: the soft alignment a decoder's attention recorded while it decoded (interface of
neuralmonkey/runners/word_alignment_runner.py:12-44).

``fetches`` is ``{"alignment": transpose(attention.histories["<decoder.name>_run"], [1, 2, 0])}`` -- the recorded attention
WEIGHTS [T, B, S] as [B, S, T] (:37-40), one [S, T] matrix per sentence; no losses; only the first session's result is
used (:18-19).  The reference's histories are nodes of its graph, there as soon as the decoder's runtime loop was built;
here the runtime loop of the decoder files them while it runs (``Attention.finalize_loop``), so the fetch evaluates that
loop first (a GreedyRunner over the same decoder shares it: one loop per run).  An attention the decoder does not query
never gets that key: the reference's KeyError, with its text (:33-35), when ``fetches`` is read."""
from typing import Any, Dict, List

from ..attention.base_attention import BaseAttention
from ..checking import check_argument_types
from ..decoders.decoder import Decoder
from ..runtime import tensor
from .base_runner import BaseRunner


class WordAlignmentRunner(BaseRunner):
    class Executable(BaseRunner.Executable):
        def collect_results(self, results: List[Dict]) -> None:
            self.set_runner_result(outputs=results[0]["alignment"], losses=[])

    def __init__(self, output_series: str, attention: BaseAttention, decoder: Decoder) -> None:
        check_argument_types()
        BaseRunner.__init__(self, output_series, attention)        # (``self.decoder`` is the attention, as in the reference)
        self._key = "{}_run".format(decoder.name)
        self._loop_owner = decoder
        feeds, params = decoder.get_dependencies()                 # the loop that records the histories must be fed
        self._feedables |= feeds
        self._parameterizeds |= params

    def _missing(self) -> KeyError:
        return KeyError("Attention has no recorded histories under key '{}'".format(self._key))

    @tensor
    def alignment(self, ctx):
        """[B, S, T]: a strided view of the recorded weights (the copy to the host lays it out)."""
        self._loop_owner.runtime_loop_result(ctx)
        if self._key not in self.decoder.histories:
            raise self._missing()
        return self.decoder.histories[self._key].permute(1, 2, 0)

    @property
    def fetches(self) -> Dict[str, Any]:
        if not any(att is self.decoder for att in getattr(self._loop_owner, "attentions", [])):
            raise self._missing()
        return {"alignment": self.alignment}

    @property
    def loss_names(self) -> List[str]:
        return []
