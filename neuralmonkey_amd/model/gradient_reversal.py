"""Gradient-reversal views of model parts (interface of neuralmonkey/model/gradient_reversal.py: ``StatefulView``,
``TemporalStatefulView``, ``SpatialStatefulView``, each built from one ``reversed_object``).

A view is what an adversarial head reads instead of the part itself: forward it IS the viewed part's tensor (the same
Fetch handle, nothing is copied); backward it multiplies the gradient it receives by -1 -- exact in floating point --
and hands it to the viewed part through ``RunContext.defer_backward``, where it is summed with what the part's plain
readers sent.  The viewed part therefore runs its backward pass once, on "friends minus adversaries".  A view has no
variables and feeds nothing; the viewed part is reached through ``dependencies``."""
from typing import List, Optional

import torch

from .. import ops
from ..checking import check_argument_types
from .stateful import SpatialStateful, Stateful, TemporalStateful


def _negated(ctx, owner, tag: str, grad: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """-grad in a persistent buffer of the view.  2-D gradients may be column slices (the kernel takes a row stride);
    higher ranks must be contiguous -- a copy through the tensor library is not an option inside a step."""
    if grad is None:
        return None
    if grad.dim() != 2 and not grad.is_contiguous():
        raise ValueError("{}: the gradient of shape {} with strides {} is not contiguous".format(
            owner, tuple(grad.shape), grad.stride()))
    out = ctx.buffer((id(owner), "reversed", tag) + tuple(grad.shape), tuple(grad.shape))
    width = grad.shape[-1]
    src = grad if grad.dim() == 2 else grad.view(-1, width)
    ops.ew("scale", src, None, out.view(-1, width), alpha=-1.0)
    return out


class _View:
    """The part all three views share."""

    def __init__(self, reversed_object) -> None:
        self._reversed_object = reversed_object

    @property
    def dependencies(self) -> List[str]:
        return ["_reversed_object"]

    def graph_safe_training(self, train_mode: bool) -> bool:
        return getattr(self._reversed_object, "graph_safe_training", lambda t: False)(train_mode)

    def backward(self, ctx, d_states: Optional[torch.Tensor], d_final: Optional[torch.Tensor] = None) -> None:
        ctx.defer_backward(self._reversed_object, _negated(ctx, self, "states", d_states),
                           _negated(ctx, self, "final", d_final))

    def __str__(self) -> str:
        return "{}({})".format(type(self).__name__, self._reversed_object)


class StatefulView(_View, Stateful):
    """``output`` / ``output_size`` of a Stateful part, gradient reversed."""
    output = property(lambda self: self._reversed_object.output)
    output_size = property(lambda self: self._reversed_object.output_size)

    def __init__(self, reversed_object: Stateful) -> None:
        check_argument_types()
        _View.__init__(self, reversed_object)


class TemporalStatefulView(_View, TemporalStateful):
    """``temporal_states`` of a TemporalStateful part, gradient reversed; mask and ``dimension`` pass through."""
    temporal_states = property(lambda self: self._reversed_object.temporal_states)
    temporal_mask = property(lambda self: self._reversed_object.temporal_mask)
    dimension = property(lambda self: self._reversed_object.dimension)

    def __init__(self, reversed_object: TemporalStateful) -> None:
        check_argument_types()
        _View.__init__(self, reversed_object)


class SpatialStatefulView(_View, SpatialStateful):
    """``spatial_states`` of a SpatialStateful part, gradient reversed; mask and ``dimension`` pass through."""
    spatial_states = property(lambda self: self._reversed_object.spatial_states)
    spatial_mask = property(lambda self: self._reversed_object.spatial_mask)
    dimension = property(lambda self: self._reversed_object.dimension)

    def __init__(self, reversed_object: SpatialStateful) -> None:
        check_argument_types()
        _View.__init__(self, reversed_object)
