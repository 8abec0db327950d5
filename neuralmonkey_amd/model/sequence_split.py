"""Split temporal states so that the sequence is n times longer (mirror of neuralmonkey/model/sequence_split.py).

``SequenceSplitter`` turns the [B, T, D] states of its ``parent`` into [B, T*factor, D/factor] ones, optionally through a
dense projection to ``projection_size`` first (tf.layers.dense: ``<name>/dense/kernel`` [D, P], ``<name>/dense/bias``
[P]).  It is the middle of the reference's non-autoregressive translation model: TransformerEncoder -> SequenceSplitter
-> TransformerEncoder -> CTCDecoder.

MI355X mapping: the projection is one taped ``F.linear`` over all B*T positions (bias and ReLU in the product's epilogue;
tanh too where nothing is recorded); the split itself is a VIEW of the contiguous [B*T, P] result as [B*T*factor,
P/factor] rows -- nothing is copied.  The mask of the longer sequence (every entry of the parent's ``factor`` times) and
its int32 lengths come from one launch that reads the parent's mask only (``ops.split_mask``, include/nmhip_split.h): no
value returns to the host, so a training step over a splitter replays as a captured graph when its parent's does.
The backward pass views the readers' summed gradient back to [B*T, P], replays the tape once and hands dL/d(parent
states) on through ``RunContext.defer_backward``: a parent with several readers still runs its backward pass once."""
from typing import Callable, List, Optional

import torch

from .. import autodiff as F
from .. import ops
from ..checking import check_argument_types
from ..nn.mlp import activation_name, declare_dense
from ..runtime import tensor
from .model_part import FeedDict, ModelPart
from .stateful import TemporalStateful

ACTIVATIONS = ("relu", "tanh", "identity")


def check_split(state_dim: int, factor: int) -> None:
    """The check of the reference's ``split_by_factor`` (sequence_split.py:81-84)."""
    if state_dim % factor != 0:
        raise ValueError((
            "Dimension of the tensor ({}) must be dividable by the given "
            "factor ({}).").format(state_dim, factor))


class _GradientSink:
    """Where the gradients of a splitter's readers meet.  Some readers defer their gradient (decoders, attentions, pooling
    encoders: ``RunContext.defer_backward``), others call ``backward`` of their input sequence themselves (recurrent and
    Transformer encoders); the tape can be replayed once only.  ``SequenceSplitter.backward`` therefore hands whatever it
    receives, from whomever, on to this object through ``defer_backward``, which sums the contributions, and the sink
    replays the tape on the sum -- once, after every reader (``input_sequence`` of the splitter is the sink, that of
    the sink the parent: the order ``RunContext.flush_backward`` derives from these)."""

    def __init__(self, splitter) -> None:
        self._splitter = splitter

    input_sequence = property(lambda self: self._splitter.parent)

    def backward(self, ctx, d_states: Optional[torch.Tensor], d_final: Optional[torch.Tensor] = None) -> None:
        self._splitter._replay(ctx, d_states)                   # pylint: disable=protected-access

    def __str__(self) -> str:
        return "{}/gradient".format(self._splitter)


class SequenceSplitter(TemporalStateful, ModelPart):
    def __init__(
            self,
            name: str,
            parent: TemporalStateful,
            factor: int,
            projection_size: int = None,
            projection_activation: Callable = None) -> None:
        """``parent``: the part whose states are split; ``factor``: by how much the sequence grows;
        ``projection_size``: width of a dense layer in front of the split (None: no layer);
        ``projection_activation``: tf.nn.relu, tf.tanh, tf.identity or None."""
        check_argument_types()
        ModelPart.__init__(self, name=name, save_checkpoint=None, load_checkpoint=None, initializers=None)
        self.parent = parent
        self.factor = factor
        self.projection_size = projection_size
        self.activation = projection_activation
        self._sink = _GradientSink(self)

        if factor < 1:
            raise ValueError("The factor ({}) must be a positive integer.".format(factor))
        if projection_size is not None and projection_size % factor != 0:
            raise ValueError((
                "Dimension of projection ({}) must be "
                "dividable by the given factor ({}).").format(
                    projection_size, factor))
        if projection_activation is not None and activation_name(projection_activation) not in ACTIVATIONS:
            raise NotImplementedError("SequenceSplitter '{}': activation {!r} is none of tf.nn.relu, tf.tanh, tf.identity"
                                      .format(name, projection_activation))

    @property
    def dependencies(self) -> List[str]:
        return super().dependencies + ["parent"]

    # RunContext.flush_backward orders the deferred backward passes by this attribute: the chain reader -> splitter ->
    # sink -> parent makes the sink wait for every reader of the splitter, and the parent for the sink.
    input_sequence = property(lambda self: self._sink)

    @property
    def _split_width(self) -> int:
        """The width that is split: the projection's, else the parent's (checked as soon as it is known)."""
        width = self.projection_size if self.projection_size else self.parent.dimension
        check_split(width, self.factor)
        return width

    @property
    def dimension(self) -> int:
        return self._split_width // self.factor

    def graph_safe_training(self, train_mode: bool) -> bool:
        return getattr(self.parent, "graph_safe_training", lambda t: False)(train_mode)

    def declare_variables(self, store) -> None:
        check_split(self._split_width, self.factor)
        if self.projection_size:
            declare_dense(self, store, "dense", self.parent.dimension, self.projection_size)

    def feed_dict(self, dataset, train: bool = True) -> FeedDict:
        return ModelPart.feed_dict(self, dataset, train)

    def stage_inputs(self, ctx) -> None:
        """Mask and lengths read fed data only (through the parent's mask): computed on every step, ahead of a step that
        is replayed as a graph."""
        self._mask_and_lengths(ctx)

    # -- forward -------------------------------------------------------------------------------------
    @tensor
    def _activations(self, ctx):
        states = self.parent.temporal_states(ctx)                            # [B,T,D]
        bsz, steps, d = states.shape
        check_split(self._split_width, self.factor)
        if not self.projection_size:
            if not states.is_contiguous():
                # a column slice of a wider buffer cannot be regrouped in place: packed by the library's strided copy
                packed = ctx.buffer((id(self), "packed", bsz, steps, d), (bsz, steps, d))
                ops.ew("copy", states.reshape(bsz * steps, d), None, packed.view(bsz * steps, d))
                states = packed
            return {"tape": None, "x": None, "out": states.view(bsz * steps, d), "shape": (bsz, steps, d)}
        train = bool(ctx.fed(self.train_mode))
        tape = F.Tape(ctx, (id(self), "split"), recording=ctx.wants_backward(train))
        x = tape.leaf(states.reshape(bsz * steps, d), needs_grad=True)
        act = activation_name(self.activation) if self.activation is not None else None
        fused = act if act == "relu" or (act == "tanh" and not tape.recording) else None
        out = F.linear(tape, x, tape.param(self, "dense/kernel"), tape.param(self, "dense/bias"), act=fused)
        if act == "tanh" and fused is None:               # (of the epilogues only relu has a backward closure)
            out = F.tanh(tape, out)
        return {"tape": tape, "x": x, "out_var": out, "out": out.data, "shape": (bsz, steps, d)}

    @tensor
    def temporal_states(self, ctx) -> torch.Tensor:
        """[B, T*factor, width/factor]: the same memory as the [B*T, width] rows."""
        act = self._activations(ctx)
        bsz, steps, _ = act["shape"]
        return act["out"].view(bsz, steps * self.factor, self.dimension)

    @tensor
    def _mask_and_lengths(self, ctx):
        mask = self.parent.temporal_mask(ctx)                                # [B,T] float
        if not mask.is_contiguous():
            raise ValueError("{}: the parent's temporal mask of shape {} with strides {} is not contiguous".format(
                self, tuple(mask.shape), mask.stride()))
        bsz, steps = mask.shape
        out = ctx.buffer((id(self), "mask", bsz, steps), (bsz, steps * self.factor))
        lengths = ctx.buffer((id(self), "len", bsz), (bsz,), torch.int32)
        return ops.split_mask(mask, self.factor, out, lengths)

    @tensor
    def temporal_mask(self, ctx) -> torch.Tensor:
        """[B, T*factor] float: every entry of the parent's mask ``factor`` times."""
        return self._mask_and_lengths(ctx)[0]

    @tensor
    def lengths(self, ctx) -> torch.Tensor:
        """[B] int32: the parent's lengths times ``factor`` (what recurrent encoders over this part read)."""
        return self._mask_and_lengths(ctx)[1]

    # -- backward ------------------------------------------------------------------------------------
    def backward(self, ctx, d_states: Optional[torch.Tensor], d_final: Optional[torch.Tensor] = None) -> None:
        """One reader's dL/d(temporal_states) [B, T*factor, width/factor]: summed with the other readers' at the sink."""
        if d_states is None:
            return
        if not d_states.is_contiguous():
            raise ValueError("{}: the gradient of shape {} with strides {} is not contiguous".format(
                self, tuple(d_states.shape), d_states.stride()))
        ctx.defer_backward(self._sink, d_states, None)

    def _replay(self, ctx, d_states: torch.Tensor) -> None:
        """The readers' summed gradient -> the gradients of the projection's variables and dL/d(parent states)
        [B, T, D], handed on.  Without a projection that is ``d_states`` itself, viewed back."""
        act = self._activations(ctx)
        bsz, steps, d = act["shape"]
        tape = act["tape"]
        if tape is None:
            ctx.defer_backward(self.parent, d_states.view(bsz, steps, d), None)
            return
        if not tape.recording:
            raise RuntimeError("SequenceSplitter.backward needs a run with train_mode=True")
        out = act["out_var"]
        out.grad = None
        F.ops.ew("copy", d_states.view(bsz * steps, self._split_width), None, tape.grad(out), accumulate=True)
        tape.backward()
        if act["x"].grad is not None:
            ctx.defer_backward(self.parent, act["x"].grad.view(bsz, steps, d), None)
