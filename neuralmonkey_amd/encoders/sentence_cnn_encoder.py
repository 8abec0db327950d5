"""Recurrent-over-convolutional sentence encoder (mirror of neuralmonkey/encoders/sentence_cnn_encoder.py).

Lee, Cho & Hofmann (2017), fully character-level NMT: dropout on the embedded characters; per filter width a
tf.nn.conv1d (stride 1, SAME) + bias + relu and a SAME max-pool over segments of ``segment_size`` positions, the widths
concatenated (cnn_encoded, :103-143); ``highway_depth`` highway layers (:145-158, nn/highway.py); a bidirectional
OrthoGRU layer over the pooled sequence with lengths ceil(len / segment_size) (:160-172); ``temporal_mask`` is the
SAME max-pool of the token mask (:188-196), which can be one position longer than those lengths -- the attention then
sees a zero state under mask 1, as in the reference.

MI355X mapping: the convolutions, the ReLU and the segment max of all widths are one launch (nm_conv1d_pool_fwd: an
implicit GEMM on the fp32 matrix cores that writes the pooled values, their argmax, the pooled mask and the pooled
lengths); a highway layer is its two products in one grouped launch plus one point-wise kernel; the GRU layer is the
taped / cluster-loop layer of RecurrentEncoder.  Everything is recorded on an autodiff tape; ``backward`` replays it.
"""
from typing import List, Optional, Tuple

import numpy as np
import torch

from .. import autodiff as F
from .. import ops
from ..checking import check_argument_types
from ..model.model_part import InitializerSpecs, ModelPart
from ..model.sequence import Sequence
from ..model.stateful import TemporalStatefulWithOutput
from ..nn.cells import make_cell
from ..runtime import tensor
from ..variables import constant_initializer, glorot_uniform_initializer, zeros_initializer
from .recurrent import RecurrentEncoder, RNNSpec


def conv_filter_initializer():
    """tf.variance_scaling_initializer(mode="fan_avg", distribution="uniform") of a conv1d filter [w, E, n]: TF's fans
    of a rank-3 shape multiply by the receptive field w (fan_in = w E, fan_out = w n)."""
    def init(rng, shape):
        receptive = int(np.prod(shape[:-2]))
        fan_in, fan_out = shape[-2] * receptive, shape[-1] * receptive
        lim = np.sqrt(3.0 / max(1.0, (fan_in + fan_out) / 2.0))
        return rng.uniform(-lim, lim, size=shape).astype(np.float32)
    return init


# pylint: disable=too-many-instance-attributes
class SentenceCNNEncoder(ModelPart, TemporalStatefulWithOutput):
    has_time_loop = True      # the GRU layer's backward pass is a latency-bound BPTT loop

    # the taped GRU layer of RecurrentEncoder, unchanged (it reads ``rnn_specs`` and ``_cells``)
    _general_layer = RecurrentEncoder._general_layer                    # pylint: disable=protected-access
    _gru_cluster_layer = RecurrentEncoder._gru_cluster_layer            # pylint: disable=protected-access
    _lstm_cluster_layer = RecurrentEncoder._lstm_cluster_layer          # pylint: disable=protected-access
    _nematus_cluster_layer = RecurrentEncoder._nematus_cluster_layer    # pylint: disable=protected-access

    # pylint: disable=too-many-arguments,too-many-locals
    def __init__(self,
                 name: str,
                 input_sequence: Sequence,
                 segment_size: int,
                 highway_depth: int,
                 rnn_size: int,
                 filters: List[Tuple[int, int]],
                 dropout_keep_prob: float = 1.0,
                 use_noisy_activations: bool = False,
                 reuse: ModelPart = None,
                 save_checkpoint: str = None,
                 load_checkpoint: str = None,
                 initializers: InitializerSpecs = None) -> None:
        ModelPart.__init__(self, name, reuse, save_checkpoint, load_checkpoint, initializers)
        check_argument_types()

        self.input_sequence = input_sequence
        self.segment_size = segment_size
        self.highway_depth = highway_depth
        self.rnn_size = rnn_size
        self.filters = filters
        self.dropout_keep_prob = dropout_keep_prob
        self.use_noisy_activations = use_noisy_activations

        if dropout_keep_prob <= 0. or dropout_keep_prob > 1.:
            raise ValueError(("Dropout keep probability must be in (0; 1], was {}").format(dropout_keep_prob))
        if rnn_size <= 0:
            raise ValueError("RNN size must be a positive integer.")
        if highway_depth <= 0:
            raise ValueError("Highway depth must be a positive integer.")
        if segment_size <= 0:
            raise ValueError("Segment size be a positive integer.")
        if not filters:
            raise ValueError("You must specify convolutional filters.")
        for filter_size, num_filters in self.filters:
            if filter_size <= 0:
                raise ValueError("Filter size must be a positive integer.")
            if num_filters <= 0:
                raise ValueError("Number of filters must be a positive int.")

        self.cnn_size = sum(n for _, n in filters)
        # tf.nn.bidirectional_dynamic_rnn's default scope (:168-172) around OrthoGRUCell
        self.rnn_specs = [RNNSpec(rnn_size, "bidirectional", "GRU")]
        self._cells = [[make_cell("GRU", self, "bidirectional_rnn/" + d, self.cnn_size, rnn_size)
                        for d in ("fw", "bw")]]

    # -- static sizes ----------------------------------------------------------------------------------
    @property
    def dimension(self) -> int:
        return 2 * self.rnn_size

    @property
    def output_size(self) -> int:
        return 2 * self.rnn_size

    def graph_safe_training(self, train_mode: bool) -> bool:
        return False

    def declare_variables(self, store) -> None:
        e = self.input_sequence.dimension
        for width, count in self.filters:
            pre = "conv-maxpool-{}".format(width)
            self.declare(store, pre + "/conv_W", (width, e, count), conv_filter_initializer())
            self.declare(store, pre + "/conv_bias", (count,), zeros_initializer())
        d = self.cnn_size
        for i in range(self.highway_depth):
            pre = "highway_layer_{}".format(i)
            self.declare(store, pre + "/weight_H", (d, d), glorot_uniform_initializer())
            self.declare(store, pre + "/bias_H", (d,), constant_initializer(-1.0))
            self.declare(store, pre + "/weight_T", (d, d), glorot_uniform_initializer())
            self.declare(store, pre + "/bias_T", (d,), constant_initializer(-1.0))
        for cell in self._cells[0]:
            cell.declare_variables(store)          # bidirectional_rnn/{fw,bw}/OrthoGRUCell/{gates,candidate}/...

    # -- forward ---------------------------------------------------------------------------------------
    @tensor
    def _activations(self, ctx):
        if self.use_noisy_activations:
            raise NotImplementedError("SentenceCNNEncoder: use_noisy_activations=True needs NoisyGRUCell, which this "
                                      "engine does not implement")
        train = bool(ctx.fed(self.train_mode))
        x_raw = self.input_sequence.temporal_states(ctx)                     # [B,S,E]
        mask = self.input_sequence.temporal_mask(ctx).contiguous()           # [B,S] float
        lengths = self.input_sequence.lengths(ctx)                           # int32 [B]
        bsz, slen, e = x_raw.shape
        tape = F.Tape(ctx, (id(self), "scnn"), recording=ctx.wants_backward(train))
        x_in = tape.leaf(x_raw.reshape(bsz * slen, e), needs_grad=True)
        x = F.dropout(tape, x_in, self.dropout_keep_prob, train, ctx.salt(self.name, "cnn_input"))
        filters = [tape.param(self, "conv-maxpool-{}/conv_W".format(w)) for w, _ in self.filters]
        biases = [tape.param(self, "conv-maxpool-{}/conv_bias".format(w)) for w, _ in self.filters]
        h, pmask, plens = F.conv1d_relu_maxpool(tape, x, filters, biases, bsz, slen, self.segment_size,
                                                mask=mask, lengths=lengths)
        sp = pmask.shape[1]
        for i in range(self.highway_depth):
            pre = "highway_layer_{}/".format(i)
            h = F.highway(tape, h, tape.param(self, pre + "weight_T"), tape.param(self, pre + "bias_T"),
                          tape.param(self, pre + "weight_H"), tape.param(self, pre + "bias_H"))
        out, final = self._general_layer(tape, h, bsz, sp, plens, 0, train)
        return {"tape": tape, "x_in": x_in, "states": out, "final": final, "mask": pmask, "lengths": plens,
                "shape": (bsz, slen, e, sp)}

    @tensor
    def temporal_states(self, ctx) -> torch.Tensor:
        act = self._activations(ctx)
        bsz, _, _, sp = act["shape"]
        return act["states"].data.view(bsz, sp, self.dimension)

    @tensor
    def temporal_mask(self, ctx) -> torch.Tensor:
        return self._activations(ctx)["mask"]

    @tensor
    def output(self, ctx) -> torch.Tensor:
        return self._activations(ctx)["final"].data

    def backward(self, ctx, d_states: Optional[torch.Tensor], d_final: Optional[torch.Tensor]) -> None:
        act = self._activations(ctx)
        tape = act["tape"]
        if not tape.recording:
            raise RuntimeError("SentenceCNNEncoder.backward needs a run with train_mode=True")
        bsz, slen, e, sp = act["shape"]
        # added into the outputs' gradient buffers, never swapped in: the step-by-step GRU tape holds views of those
        # buffers (one per time step) that its closures read
        if d_states is not None:
            ops.ew("copy", d_states.reshape(bsz * sp, -1), None, tape.grad(act["states"]), accumulate=True)
        if d_final is not None:
            ops.ew("copy", d_final, None, tape.grad(act["final"]), accumulate=True)
        tape.backward()
        if act["x_in"].grad is not None and hasattr(self.input_sequence, "backward"):
            self.input_sequence.backward(ctx, act["x_in"].grad.view(bsz, slen, e))
