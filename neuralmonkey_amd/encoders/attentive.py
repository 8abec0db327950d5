"""Structured self-attentive sentence embedding (mirror of neuralmonkey/encoders/attentive.py; Lin et al. 2017,
https://arxiv.org/abs/1703.03130).

``attention_weights`` [B,T,H] = softmax over TIME of tanh(states . S1) . S2, masked and renormalised (:60-75);
``temporal_states`` [B,H,D'] = weights^T . states (optionally projected first, :77-87) -- the "time" axis of the result
is the attention heads, so ``temporal_mask`` is all ones; ``output`` is that matrix flattened and optionally projected.

MI355X mapping: the five products are the fp32 MFMA GEMM (tanh in its epilogue outside training; the per-sentence
weights^T . states as one batched launch); the softmax along the time axis of the [B,T,H] energies is one launch of
csrc/nm_pool.hip in the energies' own layout -- no transposes.  Everything is recorded on an autodiff tape."""
from typing import Optional

import torch

from .. import autodiff as F
from .. import ops
from ..attention.base_attention import Attendable, get_attention_mask, get_attention_states
from ..checking import check_argument_types
from ..model.model_part import InitializerSpecs, ModelPart
from ..model.stateful import TemporalStateful, TemporalStatefulWithOutput
from ..runtime import tensor
from ..variables import glorot_uniform_initializer, zeros_initializer


class AttentiveEncoder(ModelPart, TemporalStatefulWithOutput):
    """``num_heads`` attention distributions over the positions of ``input_sequence``; each head's weighted sum of the
    states is one row of ``temporal_states`` [B, H, D'], their concatenation (optionally projected) is ``output``."""

    # pylint: disable=too-many-arguments
    def __init__(self,
                 name: str,
                 input_sequence: Attendable,
                 hidden_size: int,
                 num_heads: int,
                 output_size: int = None,
                 state_proj_size: int = None,
                 dropout_keep_prob: float = 1.0,
                 reuse: ModelPart = None,
                 save_checkpoint: str = None,
                 load_checkpoint: str = None,
                 initializers: InitializerSpecs = None) -> None:
        check_argument_types()
        ModelPart.__init__(self, name, reuse, save_checkpoint, load_checkpoint, initializers)

        self.input_sequence = input_sequence
        self.hidden_size = hidden_size
        self.num_heads = num_heads
        self._output_size = output_size
        self.state_proj_size = state_proj_size
        self.dropout_keep_prob = dropout_keep_prob

        if self.dropout_keep_prob <= 0.0 or self.dropout_keep_prob > 1.0:
            raise ValueError("Dropout keep prob must be inside (0,1].")
    # pylint: enable=too-many-arguments

    # -- static sizes ----------------------------------------------------------------------------------
    @property
    def dimension(self) -> int:
        return self.state_proj_size if self.state_proj_size is not None else self.input_sequence.dimension

    @property
    def output_size(self) -> int:
        return self._output_size if self._output_size is not None else self.num_heads * self.dimension

    def graph_safe_training(self, train_mode: bool) -> bool:
        return getattr(self.input_sequence, "graph_safe_training", lambda t: False)(train_mode)

    def declare_variables(self, store) -> None:
        """tf.layers.dense: glorot_uniform kernels, zero biases."""
        d = self.input_sequence.dimension
        self.declare(store, "S1/kernel", (d, self.hidden_size), glorot_uniform_initializer())
        self.declare(store, "S2/kernel", (self.hidden_size, self.num_heads), glorot_uniform_initializer())
        if self.state_proj_size is not None:
            self.declare(store, "state_projection/kernel", (d, self.state_proj_size), glorot_uniform_initializer())
            self.declare(store, "state_projection/bias", (self.state_proj_size,), zeros_initializer())
        if self._output_size is not None:
            self.declare(store, "output_projection/kernel", (self.num_heads * self.dimension, self._output_size),
                         glorot_uniform_initializer())
            self.declare(store, "output_projection/bias", (self._output_size,), zeros_initializer())

    # -- forward ---------------------------------------------------------------------------------------
    @tensor
    def _activations(self, ctx):
        train = bool(ctx.fed(self.train_mode))
        states = get_attention_states(self.input_sequence, ctx)               # [B,T,D]
        mask = get_attention_mask(self.input_sequence, ctx)                   # [B,T] float, or None
        bsz, steps, d = states.shape
        raw_shape = (bsz, steps, d)
        if not isinstance(self.input_sequence, TemporalStateful):            # a spatial map, flattened above
            raw_shape = tuple(self.input_sequence.spatial_states(ctx).shape)
        heads = self.num_heads
        tape = F.Tape(ctx, (id(self), "attentive"), recording=ctx.wants_backward(train))
        if not states.is_contiguous():
            # (the products below read [B*T, D] rows; a copy through the tensor library has no place inside a step)
            raise ValueError("AttentiveEncoder '{}': the states of '{}' (shape {}, strides {}) are not contiguous"
                             .format(self.name, self.input_sequence, tuple(states.shape), states.stride()))
        x_in = tape.leaf(states.view(bsz * steps, d), needs_grad=True)
        x = F.dropout(tape, x_in, self.dropout_keep_prob, train, ctx.salt(self.name, "attention_states"))
        if tape.recording:
            hidden = F.tanh(tape, F.linear(tape, x, tape.param(self, "S1/kernel")))
        else:
            hidden = F.linear(tape, x, tape.param(self, "S1/kernel"), act="tanh")
        energies = F.linear(tape, hidden, tape.param(self, "S2/kernel"))      # [B*T, H]
        weights = F.time_softmax(tape, energies, mask, bsz, steps)
        proj = x
        if self.state_proj_size is not None:
            proj = F.linear(tape, x, tape.param(self, "state_projection/kernel"),
                            tape.param(self, "state_projection/bias"))
        temporal = F.heads_weighted_sum(tape, weights, proj, bsz, steps)      # [B*H, D']
        width = heads * self.dimension
        output = tape.view(temporal, lambda t: t.view(bsz, width))
        if self._output_size is not None:
            output = F.linear(tape, output, tape.param(self, "output_projection/kernel"),
                              tape.param(self, "output_projection/bias"))
        ones = ctx.buffer((id(self), "ones", bsz, heads), (bsz, heads))
        ops.fill(ones, 1.0)
        return {"tape": tape, "x_in": x_in, "weights": weights, "temporal": temporal, "output": output, "ones": ones,
                "shape": (bsz, steps, d), "states_shape": raw_shape}

    @tensor
    def attention_weights(self, ctx) -> torch.Tensor:
        act = self._activations(ctx)
        bsz, steps, _ = act["shape"]
        return act["weights"].data.view(bsz, steps, self.num_heads)

    @tensor
    def temporal_states(self, ctx) -> torch.Tensor:
        act = self._activations(ctx)
        return act["temporal"].data.view(act["shape"][0], self.num_heads, self.dimension)

    @tensor
    def temporal_mask(self, ctx) -> torch.Tensor:
        return self._activations(ctx)["ones"]

    @tensor
    def output(self, ctx) -> torch.Tensor:
        return self._activations(ctx)["output"].data

    def backward(self, ctx, d_states: Optional[torch.Tensor], d_final: Optional[torch.Tensor]) -> None:
        act = self._activations(ctx)
        tape = act["tape"]
        if not tape.recording:
            raise RuntimeError("AttentiveEncoder.backward needs a run with train_mode=True")
        bsz, steps, d = act["shape"]
        if d_states is not None:
            if not d_states.is_contiguous():
                raise ValueError("AttentiveEncoder '{}': the gradient of its temporal states (shape {}, strides {}) is "
                                 "not contiguous".format(self.name, tuple(d_states.shape), d_states.stride()))
            ops.ew("copy", d_states.view(bsz * self.num_heads, self.dimension), None, tape.grad(act["temporal"]),
                   accumulate=True)
        if d_final is not None:
            ops.ew("copy", d_final, None, tape.grad(act["output"]), accumulate=True)
        tape.backward()
        grad = act["x_in"].grad
        if grad is not None and hasattr(self.input_sequence, "backward"):
            ctx.defer_backward(self.input_sequence, grad.view(*act["states_shape"]), None)
