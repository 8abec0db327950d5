"""Convolutional sequence-to-sequence encoder (mirror of neuralmonkey/encoders/facebook_conv.py; Gehring et al. 2017,
http://arxiv.org/abs/1705.03122).

``p`` = the embedded input + the first T rows of a trainable [max_length, E] table of order embeddings (:85-100; padded
positions of the embedded input are zero, so they carry the bare order embedding and nothing masks them afterwards);
x_0 = dense(p) (``order_and_embed``); ``encoder_layers`` times x_{l+1} = glu(conv1d_SAME(x_l) + bias) + x_l (:102-121,
the convolution is NOT masked: padded positions feed real ones within the receptive field); ``temporal_states`` = x_L +
dense(p) (``input_to_final_state``, :70-73); ``output`` = the maximum over all T positions, padded ones included
(:75-79); ``temporal_mask`` is the input sequence's.

MI355X mapping: the two projections of ``p`` are one grouped product where their kernels lie back to back in the
parameter buffer; a residual layer is ONE launch (nm_conv1d_glu_fwd: an implicit GEMM on the fp32 matrix cores whose
epilogue applies both biases, the sigmoid, the product and the residual add in registers); ``output`` is the pooling
kernel of csrc/nm_pool.hip under an all-ones mask.  There is no time loop.  Everything is recorded on an autodiff tape;
``backward`` replays it.
"""
from typing import Optional

import numpy as np
import torch

from .. import autodiff as F
from .. import ops
from ..checking import check_argument_types
from ..model.model_part import InitializerSpecs, ModelPart
from ..model.sequence import EmbeddedSequence
from ..model.stateful import TemporalStatefulWithOutput
from ..runtime import tensor
from ..variables import glorot_uniform_initializer, random_normal_initializer, zeros_initializer


class SentenceEncoder(ModelPart, TemporalStatefulWithOutput):
    has_time_loop = False

    # pylint: disable=too-many-arguments
    def __init__(self,
                 name: str,
                 input_sequence: EmbeddedSequence,
                 conv_features: int,
                 encoder_layers: int,
                 kernel_width: int = 5,
                 dropout_keep_prob: float = 1.0,
                 reuse: ModelPart = None,
                 save_checkpoint: str = None,
                 load_checkpoint: str = None,
                 initializers: InitializerSpecs = None) -> None:
        """``dropout_keep_prob`` is stored and never applied: the reference keeps it as an attribute (:42) and no
        dropout appears anywhere in its graph, so none is applied here either."""
        check_argument_types()
        ModelPart.__init__(self, name, reuse, save_checkpoint, load_checkpoint, initializers)

        self.input_sequence = input_sequence
        self.encoder_layers = encoder_layers
        self.conv_features = conv_features
        self.kernel_width = kernel_width
        self.dropout_keep_prob = dropout_keep_prob

        if conv_features <= 0:
            raise ValueError("Number of features must be a positive integer.")
        if encoder_layers <= 0:
            raise ValueError("Number of encoder layers must be a positive integer.")

        if self.input_sequence.max_length is None:
            raise ValueError("Input sequence must have a maximum length for "
                             "positional embeddings with this encoder")
        self.max_input_length = self.input_sequence.max_length
    # pylint: enable=too-many-arguments

    # -- static sizes ----------------------------------------------------------------------------------
    @property
    def dimension(self) -> int:
        return self.conv_features

    @property
    def output_size(self) -> int:
        return self.conv_features

    def graph_safe_training(self, train_mode: bool) -> bool:
        """Pure kernel launches on persistent buffers; the shapes depend on the batch only through T."""
        return True

    def declare_variables(self, store) -> None:
        e, c = self.input_sequence.embedding_sizes[0], self.conv_features
        # get_variable without an initializer (:89-91) and tf.layers.dense kernels: TensorFlow's default, glorot uniform
        self.declare(store, "input_projection/order_embeddings", (self.max_input_length, e), glorot_uniform_initializer())
        # (the two kernels one after the other: the projections of p are one grouped product when they are adjacent)
        self.declare(store, "order_and_embed/kernel", (e, c), glorot_uniform_initializer())
        self.declare(store, "input_to_final_state/kernel", (e, c), glorot_uniform_initializer())
        self.declare(store, "order_and_embed/bias", (c,), zeros_initializer())
        self.declare(store, "input_to_final_state/bias", (c,), zeros_initializer())
        for i in range(self.encoder_layers):
            pre = "encoder_conv_{}/".format(i)
            self.declare(store, pre + "convolution_filters", (self.kernel_width, c, 2 * c),
                         random_normal_initializer(stddev=float(np.sqrt(4 / c))))          # :106-111
            self.declare(store, pre + "conv_bias", (2 * c,), zeros_initializer())

    # -- forward ---------------------------------------------------------------------------------------
    @tensor
    def _activations(self, ctx):
        train = bool(ctx.fed(self.train_mode))
        x_raw = self.input_sequence.temporal_states(ctx)                     # [B,T,E]
        bsz, steps, e = x_raw.shape
        if e != self.input_sequence.embedding_sizes[0]:
            raise ValueError("SentenceEncoder '{}': the order embeddings have the width of the first factor ({}), the "
                             "input sequence has {}".format(self.name, self.input_sequence.embedding_sizes[0], e))
        tape = F.Tape(ctx, (id(self), "convs2s"), recording=ctx.wants_backward(train))
        x_in = tape.leaf(x_raw.reshape(bsz * steps, e), needs_grad=True)
        table = tape.param(self, "input_projection/order_embeddings")
        p = F.add_position_param(tape, x_in, table, bsz, steps)              # ordered_embedded_inputs (:93-100)
        first, last = F.linear_multi(tape, p, [tape.param(self, "order_and_embed/kernel"),
                                               tape.param(self, "input_to_final_state/kernel")])
        x = F.add_row(tape, first, tape.param(self, "order_and_embed/bias"))
        for i in range(self.encoder_layers):
            pre = "encoder_conv_{}/".format(i)
            x = F.conv1d_glu(tape, x, tape.param(self, pre + "convolution_filters"), tape.param(self, pre + "conv_bias"),
                             bsz, steps)
        states = F.add_row(tape, F.add(tape, x, last), tape.param(self, "input_to_final_state/bias"))
        out = F.time_max(tape, states, bsz, steps)
        return {"tape": tape, "x_in": x_in, "p": p, "states": states, "output": out, "shape": (bsz, steps, e)}

    @tensor
    def ordered_embedded_inputs(self, ctx) -> torch.Tensor:
        act = self._activations(ctx)
        bsz, steps, e = act["shape"]
        return act["p"].data.view(bsz, steps, e)

    @tensor
    def temporal_states(self, ctx) -> torch.Tensor:
        act = self._activations(ctx)
        bsz, steps, _ = act["shape"]
        return act["states"].data.view(bsz, steps, self.conv_features)

    @tensor
    def temporal_mask(self, ctx) -> torch.Tensor:
        return self.input_sequence.temporal_mask(ctx)

    @tensor
    def output(self, ctx) -> torch.Tensor:
        return self._activations(ctx)["output"].data

    def backward(self, ctx, d_states: Optional[torch.Tensor], d_final: Optional[torch.Tensor]) -> None:
        act = self._activations(ctx)
        tape = act["tape"]
        if not tape.recording:
            raise RuntimeError("SentenceEncoder.backward needs a run with train_mode=True")
        bsz, steps, e = act["shape"]
        if d_states is not None:
            ops.ew("copy", d_states.reshape(bsz * steps, -1), None, tape.grad(act["states"]), accumulate=True)
        if d_final is not None:
            ops.ew("copy", d_final, None, tape.grad(act["output"]), accumulate=True)
        tape.backward()
        if act["x_in"].grad is not None and hasattr(self.input_sequence, "backward"):
            self.input_sequence.backward(ctx, act["x_in"].grad.view(bsz, steps, e))
