"""Pooling of a sequence into one vector (mirror of neuralmonkey/encoders/pooling.py).

``SequenceMaxPooling``: ``output`` = max over time of states * mask + 1e-15 * (1 - mask) (:44-51) -- padded positions
contribute 1e-15, not -inf, so a feature that is negative at every real position pools to 1e-15 whenever its sentence
has padding.  ``SequenceAveragePooling``: sum(states * mask) / (sum(mask) + 1e-8) (:60-63).

MI355X mapping: one launch of csrc/nm_pool.hip each way (a thread owns 4 adjacent features, the waves of a workgroup
split the time axis and combine in LDS in a fixed order).  The maximum also leaves the number of positions that hold it,
the count the gradient of tf.reduce_max divides by.  Nothing reads the device from the host: the reference's assertion
that the batch holds at least one token is made on the fed host arrays."""
from typing import Optional

import numpy as np
import torch

from .. import ops
from ..checking import check_argument_types
from ..model.model_part import InitializerSpecs, ModelPart
from ..model.stateful import Stateful, TemporalStateful
from ..runtime import tensor


# pylint: disable=abstract-method
class SequencePooling(ModelPart, Stateful):
    """Base of the two poolers: [B, T, D] states of ``input_sequence`` -> one [B, D] ``output``; ``MODE`` names the
    reduction of csrc/nm_pool.hip that a subclass stands for."""
    MODE: Optional[str] = None

    def __init__(self,
                 name: str,
                 input_sequence: TemporalStateful,
                 reuse: ModelPart = None,
                 save_checkpoint: str = None,
                 load_checkpoint: str = None,
                 initializers: InitializerSpecs = None) -> None:
        check_argument_types()
        ModelPart.__init__(self, name, reuse, save_checkpoint, load_checkpoint, initializers)
        self.input_sequence = input_sequence

    @property
    def output_size(self) -> int:
        return self.input_sequence.dimension

    def graph_safe_training(self, train_mode: bool) -> bool:
        return getattr(self.input_sequence, "graph_safe_training", lambda t: False)(train_mode)

    def check_fed_mask(self, ctx) -> None:
        """Host-side checks of the fed batch (none here)."""

    def stage_inputs(self, ctx) -> None:
        """Runs on EVERY training step, before a captured step is replayed: host code a replayed graph would skip."""
        self.check_fed_mask(ctx)

    @tensor
    def _pooled(self, ctx):
        if self.MODE is None:
            raise NotImplementedError("Abstract property")
        self.check_fed_mask(ctx)
        states = self.input_sequence.temporal_states(ctx)                    # [B,T,D]
        mask = self.input_sequence.temporal_mask(ctx)                        # [B,T] float
        bsz, steps, d = states.shape
        out = ctx.buffer((id(self), "pooled", bsz, d), (bsz, d))
        ties = ctx.buffer((id(self), "ties", bsz, d), (bsz, d), torch.int32) if self.MODE == "max" else None
        ops.pool_fwd(self.MODE, states, mask, out, ties)
        return {"states": states, "mask": mask, "out": out, "ties": ties}

    @tensor
    def output(self, ctx) -> torch.Tensor:
        return self._pooled(ctx)["out"]

    def backward(self, ctx, d_states: Optional[torch.Tensor], d_final: Optional[torch.Tensor]) -> None:
        """dL/d(output) [B,D] -> dL/d(the input's temporal states) [B,T,D], handed on to the input sequence."""
        if d_final is None:
            return
        act = self._pooled(ctx)
        states = act["states"]
        dx = ctx.buffer((id(self), "d_states") + tuple(states.shape), tuple(states.shape))
        ops.pool_bwd(self.MODE, d_final, act["mask"], dx, x=states if self.MODE == "max" else None,
                     out=act["out"] if self.MODE == "max" else None, ties=act["ties"])
        ctx.defer_backward(self.input_sequence, dx, None)
# pylint: enable=abstract-method


class SequenceMaxPooling(SequencePooling):
    """``output`` [B, D] = the feature-wise maximum over the real positions, padded positions standing in as 1e-15."""
    MODE = "max"

    def check_fed_mask(self, ctx) -> None:
        """tf.assert_greater(tf.reduce_sum(mask), 0.5) (:48-49) on the fed arrays.  Covered: input sequences whose
        mask ``host_temporal_mask`` can derive on the host -- an embedded sequence or a TemporalFiller, directly or
        under recurrent / Transformer encoders.  Behind any other part (a sentence-CNN encoder, another view) the
        mask exists on the device only; reading it back would end graph capture, so the check is NOT made there and
        a batch without tokens pools to 1e-15 everywhere instead of raising."""
        from ..decoders.sequence_labeler import host_temporal_mask
        host = host_temporal_mask(self.input_sequence, ctx)
        if host is not None and not float(np.sum(host)) > 0.5:
            raise ValueError("SequenceMaxPooling '{}': the batch holds no token (the sum of the input mask must be "
                             "greater than 0.5)".format(self.name))


class SequenceAveragePooling(SequencePooling):
    """``output`` [B, D] = the feature-wise mean over the real positions (zeros for an empty sentence)."""
    MODE = "avg"
