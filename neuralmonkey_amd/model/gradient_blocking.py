"""Gradient-blocking views of model parts (interface of neuralmonkey/model/gradient_blocking.py: ``StatefulView``,
``TemporalStatefulView``, ``SpatialStatefulView``, each built from one ``blocked_object``).

A view is what a second head reads when the part under it is to stay as it is (``tf.stop_gradient``): forward it IS the
viewed part's tensor (the same Fetch handle, nothing is copied); backward it hands NOTHING on.  Readers send their
gradient to the view through ``RunContext.defer_backward`` like to any other part, and it ends there: the viewed part
receives what its plain readers sent and nothing else, so its gradient is bit for bit the one of the model without the
view.  A part that is read through blocking views only never runs its backward pass.  Its slices of the flat gradient
are then the zeros every step starts from (``GenericTrainer._objective_gradients`` clears the buffer before the first
launch of a step, replayed as a graph or not; ``DelayedUpdateTrainer`` adds that cleared buffer to its sum; the
data-parallel exchange sums the ranks' zeros): the optimizer sees a zero gradient plus the part's L1 / L2 terms, as
TensorFlow's does for a variable behind ``tf.stop_gradient``.  A view has no variables and feeds nothing; the viewed
part is reached through ``dependencies``."""
from typing import List, Optional

import torch

from ..checking import check_argument_types
from .stateful import SpatialStateful, Stateful, TemporalStateful


class _View:
    """The part all three views share."""

    def __init__(self, blocked_object) -> None:
        self._blocked_object = blocked_object

    @property
    def dependencies(self) -> List[str]:
        return ["_blocked_object"]

    def graph_safe_training(self, train_mode: bool) -> bool:
        return getattr(self._blocked_object, "graph_safe_training", lambda t: False)(train_mode)

    def backward(self, ctx, d_states: Optional[torch.Tensor], d_final: Optional[torch.Tensor] = None) -> None:
        """tf.stop_gradient: the gradient ends here."""

    def __str__(self) -> str:
        return "{}({})".format(type(self).__name__, self._blocked_object)


class StatefulView(_View, Stateful):
    """``output`` / ``output_size`` of a Stateful part, gradient blocked."""
    output = property(lambda self: self._blocked_object.output)
    output_size = property(lambda self: self._blocked_object.output_size)

    def __init__(self, blocked_object: Stateful) -> None:
        check_argument_types()
        _View.__init__(self, blocked_object)


class TemporalStatefulView(_View, TemporalStateful):
    """``temporal_states`` of a TemporalStateful part, gradient blocked; mask and ``dimension`` pass through."""
    temporal_states = property(lambda self: self._blocked_object.temporal_states)
    temporal_mask = property(lambda self: self._blocked_object.temporal_mask)
    dimension = property(lambda self: self._blocked_object.dimension)

    def __init__(self, blocked_object: TemporalStateful) -> None:
        check_argument_types()
        _View.__init__(self, blocked_object)


class SpatialStatefulView(_View, SpatialStateful):
    """``spatial_states`` of a SpatialStateful part, gradient blocked; mask and ``dimension`` pass through."""
    spatial_states = property(lambda self: self._blocked_object.spatial_states)
    spatial_mask = property(lambda self: self._blocked_object.spatial_mask)
    dimension = property(lambda self: self._blocked_object.dimension)

    def __init__(self, blocked_object: SpatialStateful) -> None:
        check_argument_types()
        _View.__init__(self, blocked_object)
