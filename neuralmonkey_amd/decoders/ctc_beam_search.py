"""CTC prefix beam search as a decoding mode of a ``CTCDecoder``.

The reference decodes ``beam_width != 1`` with ``tf.nn.ctc_beam_search_decoder`` (decoders/ctc_decoder.py:76-89); here
that search is a decoder of its own that wraps the CTC head the way ``BeamSearchDecoder`` wraps an autoregressive one.
Greedy decoding takes the best class of every frame and so follows ONE alignment; the beam search sums, per label
prefix, the alignments that end in blank and those that end in the prefix's last label, and keeps the ``beam_size``
prefixes of largest total (include/nmhip_ctc_beam.h states the recurrence, DESIGN 4.8b the kernels).

``decoded`` has the shape contract of ``CTCDecoder.decoded`` -- [max(1, longest), B] int32, time-major, padded with
END_TOKEN_INDEX -- so ``PlainRunner(output_series, decoder=<this part>)`` works unchanged; the losses are the parent's.
Both kernels run in one call (csrc/nm_ctc_beam.hip) on the parent's strided logits view; only the emitted lengths
cross to the host, for the width, as on the greedy path.
"""
import numpy as np
import torch

from .. import ops
from ..model.model_part import ModelPart
from ..runtime import tensor
from ..vocabulary import END_TOKEN_INDEX, Vocabulary
from .ctc_decoder import CTCDecoder

MAX_BEAM_SIZE = 64        # a beam slot is a lane of the frame scan's wavefront; the bound BeamSearchDecoder has


class CTCBeamSearchDecoder(ModelPart):
    def __init__(self, name: str, parent_decoder: CTCDecoder, beam_size: int,
                 merge_repeated_outputs: bool = None) -> None:
        ModelPart.__init__(self, name)
        if beam_size < 1 or beam_size > MAX_BEAM_SIZE:
            raise ValueError("beam_size must be between 1 and {}, was {}".format(MAX_BEAM_SIZE, beam_size))
        self.parent_decoder = parent_decoder
        self.beam_size = beam_size
        self.merge_repeated_outputs = (parent_decoder.merge_repeated_outputs if merge_repeated_outputs is None
                                       else bool(merge_repeated_outputs))

    @property
    def vocabulary(self) -> Vocabulary:
        return self.parent_decoder.vocabulary

    def graph_safe_training(self, train_mode: bool) -> bool:
        return False          # the emitted width of ``decoded`` is read on the host

    @tensor
    def _search(self, ctx):
        """(tokens [B, T] int32, emitted lengths [B] int32, scores [B]) on the device; None without a frame."""
        dec = self.parent_decoder
        logits = dec.logits(ctx)
        steps, bsz, _ = logits.shape
        if steps == 0:
            return None
        key = (id(self), "ctc_beam", bsz, steps)
        tokens = ctx.buffer(key + ("tokens",), (bsz, steps), torch.int32)
        out_len = ctx.buffer(key + ("out_len",), (bsz,), torch.int32)
        score = ctx.buffer(key + ("score",), (bsz,))
        ops.ctc_beam_search(logits, dec.frame_lengths(ctx), self.beam_size, self.merge_repeated_outputs, END_TOKEN_INDEX,
                            tokens, out_len, score)
        return tokens, out_len, score

    @tensor
    def decoded(self, ctx):
        """[max(1, longest emitted sequence), B] int32, padded with END_TOKEN_INDEX (``CTCDecoder.decoded``)."""
        found = self._search(ctx)
        if found is None:
            return np.full((1, int(ctx.fed(self.batch_size))), END_TOKEN_INDEX, dtype=np.int32)
        tokens, out_len, _ = found
        width = max(1, int(np.max(ctx.session.read_small(out_len), initial=0)))      # B int32 words to the host
        return tokens[:, :width].t()

    @tensor
    def scores(self, ctx) -> torch.Tensor:
        """[B] float32: the log-probability of every sentence's decoded prefix (0 for a sentence without a frame)."""
        found = self._search(ctx)
        if found is None:
            return torch.zeros(int(ctx.fed(self.batch_size)), device=ctx.device)
        return found[2]

    # -- the losses PlainRunner fetches are the parent's ----------------------------------------------------------
    @property
    def cost(self):
        return self.parent_decoder.cost

    @property
    def train_loss(self):
        return self.parent_decoder.train_loss

    @property
    def runtime_loss(self):
        return self.parent_decoder.runtime_loss
