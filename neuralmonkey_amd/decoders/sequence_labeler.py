"""Sequence labelling heads (mirror of neuralmonkey/decoders/sequence_labeler.py).

``SequenceLabeler``: ``logits`` [B,T,K] = states . logits/kernel + logits/bias over the encoders' temporal states
concatenated along the features (:93-112; with ``hidden_dim`` through tf.layers.dense + ``activation`` + dropout
first); ``train_xents`` = sparse softmax cross entropy * sentence_mask(train_targets) (:122-129 -- the mask of the
TARGETS, not of the encoder); ``cost`` = sum(xents) / (sum(mask) + 1e-9); ``decoded`` = tf.argmax(logits, 2).
``EmbeddingsLabeler``: the logits are states . embedding_matrix^T of an embedded sequence (:192-214), the masked-LM
head of tests/bert.ini.

MI355X mapping: the products are the fp32 MFMA GEMM (relu in its epilogue); everything a row of logits is asked for
-- cross entropy, gradient (in place, scaled by the trainer's device-side ``grad_scale``), argmax, log-probabilities and
the runner's masked labels -- is one launch of csrc/nm_label.hip (one wavefront per row, no LDS), or of the
vocabulary-row kernels above ``ops.label_rows_max_classes()`` classes.  Nothing of the pass reads the device from the
host, so a training step over graph-safe encoders is captured as a HIP graph.
"""
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

from .. import autodiff as F
from .. import ops
from .. import tf_shim
from ..checking import check_argument_types
from ..model.model_part import FeedDict, InitializerSpecs, ModelPart
from ..model.sequence import EmbeddedSequence, cached_index
from ..model.stateful import TemporalStateful
from ..runtime import Placeholder, tensor
from ..variables import glorot_uniform_initializer, zeros_initializer
from ..vocabulary import END_TOKEN_INDEX, PAD_TOKEN_INDEX, Vocabulary, sentence_mask
from .decoder import TrainResult

ACTIVATIONS = ("relu", "tanh", "identity")


def host_temporal_mask(encoder, ctx) -> Optional[np.ndarray]:
    """The encoder's temporal mask from the FED host arrays, where the encoder is known to hand its input sequence's
    mask through (recurrent and Transformer encoders over an embedded sequence or a TemporalFiller); None otherwise."""
    from ..encoders.numpy_stateful_filler import TemporalFiller
    from ..encoders.recurrent import RecurrentEncoder
    from ..encoders.transformer import TransformerEncoder
    from ..model.sequence import EmbeddedFactorSequence
    part = encoder
    while isinstance(part, (RecurrentEncoder, TransformerEncoder)):
        part = part.input_sequence
    if isinstance(part, EmbeddedFactorSequence) and ctx.is_fed(part.input_factors[0]):
        return sentence_mask(ctx.fed(part.input_factors[0]))
    if isinstance(part, TemporalFiller) and ctx.is_fed(part.lengths_input) and ctx.is_fed(part.states_input):
        steps = np.shape(ctx.fed(part.states_input))[1]
        return (np.arange(steps)[None, :] < np.asarray(ctx.fed(part.lengths_input))[:, None]).astype(np.float32)
    return None


class SequenceLabeler(ModelPart):
    """Classifier assigning a label to each encoder's state."""

    # pylint: disable=too-many-arguments,too-many-locals
    def __init__(self,
                 name: str,
                 encoders: List[TemporalStateful],
                 vocabulary: Vocabulary,
                 data_id: str,
                 max_output_len: int = None,
                 hidden_dim: int = None,
                 activation: Callable = tf_shim.nn.relu,
                 dropout_keep_prob: float = 1.0,
                 add_start_symbol: bool = False,
                 add_end_symbol: bool = False,
                 reuse: ModelPart = None,
                 save_checkpoint: str = None,
                 load_checkpoint: str = None,
                 initializers: InitializerSpecs = None) -> None:
        check_argument_types()
        ModelPart.__init__(self, name, reuse, save_checkpoint, load_checkpoint, initializers)

        self.encoders = encoders
        self.vocabulary = vocabulary
        self.data_id = data_id
        self.max_output_len = max_output_len
        self.hidden_dim = hidden_dim
        self.activation = activation
        self.dropout_keep_prob = dropout_keep_prob
        self.add_start_symbol = add_start_symbol
        self.add_end_symbol = add_end_symbol
        self.train_tokens = Placeholder("{}/target_tokens".format(name))
        if hidden_dim is not None and self.activation_name not in ACTIVATIONS:
            raise NotImplementedError("SequenceLabeler '{}': activation {!r} is none of tf.nn.relu, tf.tanh, tf.identity"
                                      .format(name, activation))
    # pylint: enable=too-many-arguments,too-many-locals

    @property
    def activation_name(self) -> Optional[str]:
        return getattr(self.activation, "nm_name", None)

    @property
    def input_types(self) -> Dict[str, type]:
        return {self.data_id: str}

    @property
    def input_shapes(self) -> Dict[str, List]:
        return {self.data_id: [None, None]}

    @property
    def input_dimension(self) -> int:
        return sum(enc.dimension for enc in self.encoders)

    @property
    def states_dimension(self) -> int:
        return self.input_dimension if self.hidden_dim is None else self.hidden_dim

    def graph_safe_training(self, train_mode: bool) -> bool:
        return all(getattr(e, "graph_safe_training", lambda t: False)(train_mode) for e in self.encoders)

    def declare_variables(self, store) -> None:
        if self.hidden_dim is not None:                         # tf.layers.dense: glorot_uniform kernel, zero bias
            self.declare(store, "hidden_layer/kernel", (self.input_dimension, self.hidden_dim),
                         glorot_uniform_initializer())
            self.declare(store, "hidden_layer/bias", (self.hidden_dim,), zeros_initializer())
        self._declare_logit_variables(store)

    def _declare_logit_variables(self, store) -> None:
        classes = len(self.vocabulary)
        self.declare(store, "logits/kernel", (self.states_dimension, classes), glorot_uniform_initializer())
        self.declare(store, "logits/bias", (classes,), zeros_initializer())

    # -- fed data ----------------------------------------------------------------------------------
    def feed_dict(self, dataset, train: bool = False) -> FeedDict:
        fd = ModelPart.feed_dict(self, dataset, train)
        if dataset.maybe_get_series(self.data_id) is not None:      # (no error without targets: the reference has none)
            fd[self.train_tokens] = cached_index(dataset, self.data_id, self.vocabulary, self.max_output_len,
                                                 self.add_start_symbol, self.add_end_symbol)
        return fd

    def has_targets(self, ctx) -> bool:
        return ctx.is_fed(self.train_tokens)

    @tensor
    def train_targets(self, ctx) -> torch.Tensor:
        """[B,T] int32 on the device."""
        sess = ctx.session
        return sess.staged((id(self), "label_targets"), sess.to_device(ctx.fed(self.train_tokens), torch.int32,
                                                                       "label_targets"))

    @tensor
    def train_mask(self, ctx) -> torch.Tensor:
        """[B,T] float: sentence_mask(train_targets)."""
        sess = ctx.session
        return sess.staged((id(self), "label_mask"), sess.to_device(ctx.fed(self.train_tokens), torch.float32,
                                                                    "label_mask", sentence_mask))

    def stage_inputs(self, ctx) -> None:
        """Runs on EVERY training step, before a captured step is replayed: the comparison of the encoders' masks is
        host code, which a replayed graph would not run again."""
        if len(self.encoders) > 1:
            self.input_mask(ctx)
        if self.has_targets(ctx):
            self.train_targets(ctx)

    def train_token_count(self, ctx) -> float:
        """Denominator of the cost: sum(train_mask), the number of non-pad targets."""
        return float(sentence_mask(ctx.fed(self.train_tokens)).sum())

    # -- forward -------------------------------------------------------------------------------------
    @tensor
    def input_mask(self, ctx) -> torch.Tensor:
        """The first encoder's temporal mask; the others' must equal it (:60-71).  Compared on the fed host arrays
        where the encoders hand their input's mask through, by shape otherwise: the device is not read back."""
        main = self.encoders[0]
        mask_main = main.temporal_mask(ctx)
        host_main = host_temporal_mask(main, ctx)
        for enc in self.encoders[1:]:
            mask = enc.temporal_mask(ctx)
            host = host_temporal_mask(enc, ctx)
            same = tuple(mask.shape) == tuple(mask_main.shape)
            if same and host is not None and host_main is not None:
                same = np.array_equal(host, host_main)
            if not same:
                raise ValueError("Encoders '{}' and '{}' does not have equal temporal masks.".format(str(main), str(enc)))
        return mask_main

    def _states(self, tape: F.Tape, ctx, leaves: List[F.Var], train: bool) -> F.Var:
        cat = F.concat(tape, leaves)                                 # concatenated_inputs (:93-98)
        if self.hidden_dim is None:
            return cat
        act = self.activation_name
        hidden = F.linear(tape, cat, tape.param(self, "hidden_layer/kernel"), tape.param(self, "hidden_layer/bias"),
                          act="relu" if act == "relu" else None)
        if act == "tanh":
            hidden = F.tanh(tape, hidden)
        return F.dropout(tape, hidden, self.dropout_keep_prob, train, ctx.salt(self.name, "hidden_layer"))

    def _logits(self, tape: F.Tape, ctx, states: F.Var, train: bool) -> F.Var:
        return F.linear(tape, states, tape.param(self, "logits/kernel"), tape.param(self, "logits/bias"))

    def _forward(self, ctx, want_grad: bool, grad_scale: Optional[torch.Tensor], tag: str, with_loss: bool):
        train = bool(ctx.fed(self.train_mode))
        mask = self.input_mask(ctx)                                  # validates the encoders' masks first (:96)
        bsz, steps = mask.shape
        targets = None
        if with_loss:                                                # (checked before any kernel of the pass runs)
            targets = self.train_targets(ctx)
            if tuple(targets.shape) != (bsz, steps):
                raise ValueError("SequenceLabeler '{}': the targets '{}' are {} wide, the encoder has {} steps (batch {} "
                                 "against {}): labels and states must line up one to one"
                                 .format(self.name, self.data_id, targets.shape[1], steps, targets.shape[0], bsz))
        tape = F.Tape(ctx, (id(self), tag), recording=want_grad)
        leaves, shapes = [], []
        for enc in self.encoders:
            st = enc.temporal_states(ctx)                            # [B,T,D]
            shapes.append(tuple(st.shape))
            leaves.append(tape.leaf(st.reshape(st.shape[0] * st.shape[1], st.shape[2]), needs_grad=True))
        if any(s[:2] != (bsz, steps) for s in shapes):
            raise ValueError("SequenceLabeler '{}': the encoders' temporal states {} and mask {} differ in batch or "
                             "time".format(self.name, shapes, tuple(mask.shape)))
        states = self._states(tape, ctx, leaves, train)
        logits = self._logits(tape, ctx, states, train)             # [B*T, K], batch-major rows
        rows = bsz * steps
        saved = {"tape": tape, "leaves": leaves, "shapes": shapes, "bsz": bsz, "steps": steps, "logits": logits.data,
                 "dlogits": logits.data if want_grad and with_loss else None, "loss_rows": None}
        argmax = labels = None
        if not want_grad:            # a training step wants loss and gradient only
            argmax = saved["argmax"] = ctx.buffer((id(self), tag, "argmax", rows), (rows,), torch.int32)
            labels = saved["labels"] = ctx.buffer((id(self), tag, "labels", rows), (rows,), torch.int32)
        loss_rows = F.label_xent(tape, logits, None if targets is None else targets.reshape(-1), PAD_TOKEN_INDEX,
                                 grad_scale, None, argmax, mask.reshape(-1), END_TOKEN_INDEX, labels)
        loss_sum, count = None, 0.0
        if with_loss:
            saved["loss_rows"] = loss_rows
            loss_sum = ctx.buffer((id(self), tag, "loss_sum"), (1,))
            ops.reduce_sum(loss_rows, loss_sum)
            count = self.train_token_count(ctx)
        return TrainResult(loss_sum, count, steps, saved)

    # -- the interface GenericTrainer._objective_gradients calls ----------------------------------------
    def _train_loop(self, ctx, want_grad: bool = False, grad_scale: Optional[torch.Tensor] = None) -> TrainResult:
        return self._forward(ctx, want_grad, grad_scale, "label_train", True)

    def backward(self, ctx, res: TrainResult) -> None:
        sv = res.saved
        sv["tape"].backward()
        for enc, var, shape in zip(self.encoders, sv["leaves"], sv["shapes"]):
            if var.grad is not None:
                ctx.defer_backward(enc, var.grad.view(*shape), None)

    # -- fetchable surface (the reference's @tensor names) ------------------------------------------------
    @tensor
    def train_loop_result(self, ctx) -> TrainResult:
        return self._train_loop(ctx)

    @tensor
    def _inference(self, ctx) -> TrainResult:
        """The pass without targets, or beside a training pass whose logits became their gradient."""
        key = self.train_loop_result.key
        if key in ctx.memo and ctx.memo[key].saved["dlogits"] is None:
            return ctx.memo[key]
        if self.has_targets(ctx) and key not in ctx.memo:
            return self.train_loop_result(ctx)
        return self._forward(ctx, False, None, "label_run", False)

    def _result(self, ctx) -> TrainResult:
        return self._inference(ctx)

    @tensor
    def logits(self, ctx) -> torch.Tensor:
        sv = self._result(ctx).saved
        return sv["logits"].view(sv["bsz"], sv["steps"], -1)

    @tensor
    def logprobs(self, ctx) -> torch.Tensor:
        """[B,T,K] tf.nn.log_softmax(logits): a call of its own, made only when somebody fetches it."""
        logits = self.logits(ctx)
        bsz, steps, k = logits.shape
        out = ctx.buffer((id(self), "logprobs", bsz, steps, k), (bsz * steps, k))
        ops.label_rows(logits.view(bsz * steps, k), logprobs=out)
        return out.view(bsz, steps, k)

    @tensor
    def decoded(self, ctx) -> torch.Tensor:
        """[B,T] int32: tf.argmax(logits, 2), the first maximum."""
        sv = self._result(ctx).saved
        return sv["argmax"].view(sv["bsz"], sv["steps"])

    @tensor
    def labels(self, ctx) -> torch.Tensor:
        """[B,T] int32: ``decoded`` where ``input_mask`` is set, END_TOKEN_INDEX elsewhere -- what LabelRunner turns
        into sentences (runners/label_runner.py:34-39), computed by the same kernel on the device."""
        sv = self._result(ctx).saved
        return sv["labels"].view(sv["bsz"], sv["steps"])

    @tensor
    def train_xents(self, ctx) -> torch.Tensor:
        """[B,T]: cross entropy, exactly zero where the target is <pad> (XentRunner)."""
        res = self.train_loop_result(ctx)
        return res.saved["loss_rows"].view(res.saved["bsz"], res.saved["steps"])

    @tensor
    def cost(self, ctx):
        """sum(train_xents) / (sum(train_mask) + 1e-9); in fp32 the 1e-9 only matters for an empty mask: cost 0."""
        if not self.has_targets(ctx):
            return 0.0
        res = self.train_loop_result(ctx)
        out = ctx.buffer((id(self), "cost"), (1,))
        alpha = 1.0 / res.token_count if res.token_count else 0.0
        return ops.ew("scale", res.loss_sum[0:1], None, out, alpha=alpha)[0]

    @property
    def train_loss(self):
        return self.cost

    @property
    def runtime_loss(self):
        return self.cost


class EmbeddingsLabeler(SequenceLabeler):
    """SequenceLabeler that uses an embedding matrix for output projection."""

    # pylint: disable=too-many-arguments,too-many-locals
    def __init__(self,
                 name: str,
                 encoders: List[TemporalStateful],
                 embedded_sequence: EmbeddedSequence,
                 data_id: str,
                 max_output_len: int = None,
                 hidden_dim: int = None,
                 activation: Callable = tf_shim.nn.relu,
                 train_embeddings: bool = True,
                 dropout_keep_prob: float = 1.0,
                 add_start_symbol: bool = False,
                 add_end_symbol: bool = False,
                 reuse: ModelPart = None,
                 save_checkpoint: str = None,
                 load_checkpoint: str = None,
                 initializers: InitializerSpecs = None) -> None:
        check_argument_types()
        SequenceLabeler.__init__(
            self, name, encoders, embedded_sequence.vocabulary, data_id, max_output_len, hidden_dim=hidden_dim,
            activation=activation, dropout_keep_prob=dropout_keep_prob, add_start_symbol=add_start_symbol,
            add_end_symbol=add_end_symbol, reuse=reuse, save_checkpoint=save_checkpoint,
            load_checkpoint=load_checkpoint, initializers=initializers)

        self.embedded_sequence = embedded_sequence
        self.train_embeddings = train_embeddings
    # pylint: enable=too-many-arguments,too-many-locals

    @property
    def dependencies(self) -> List[str]:
        return ModelPart.dependencies.fget(self) + ["embedded_sequence"]

    @property
    def embedding_dimension(self) -> int:
        return self.embedded_sequence.embedding_sizes[0]

    def _declare_logit_variables(self, store) -> None:
        if self.states_dimension != self.embedding_dimension:       # (:204-207)
            self.declare(store, "project_for_embeddings/kernel", (self.states_dimension, self.embedding_dimension),
                         glorot_uniform_initializer())
            self.declare(store, "project_for_embeddings/bias", (self.embedding_dimension,), zeros_initializer())

    def _logits(self, tape: F.Tape, ctx, states: F.Var, train: bool) -> F.Var:
        name = self.embedded_sequence.embedding_matrix_name
        # the head's share of the table's gradient ADDS into the shared table's gradient, beside the scatter-add of the
        # encoder's input; tf.stop_gradient (train_embeddings=False) cuts this share only
        learn = self.train_embeddings and getattr(self.embedded_sequence, "trainable", True)
        table = tape.named_param(name) if learn else F.Var(ctx.store[name], None, False)
        if self.states_dimension != self.embedding_dimension:
            states = F.linear(tape, states, tape.param(self, "project_for_embeddings/kernel"),
                              tape.param(self, "project_for_embeddings/bias"))
            states = F.dropout(tape, states, self.dropout_keep_prob, train,
                               ctx.salt(self.name, "project_for_embeddings"))
        return F.linear(tape, states, table, None, trans_b=True)
