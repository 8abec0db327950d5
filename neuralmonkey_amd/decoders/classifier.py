"""``Classifier``: an MLP over the encoders' ``output`` vectors (mirror of neuralmonkey/decoders/classifier.py).

The API pretends it is an RNN decoder which always generates a sequence of length exactly one: ``decoded_seq`` is
[1,B], ``decoded_logits`` and ``runtime_logprobs`` are [1,B,K].  The loss is the batch mean of the sparse softmax cross
entropy (:104-107) -- every row counts, also one whose label is index 0.

MI355X mapping: the layers are the fp32 MFMA GEMM (relu in its epilogue); cross entropy, its gradient in place (scaled
by the trainer's device-side ``grad_scale`` = weight / B), and the argmax of a row are one launch of csrc/nm_label.hip
with a pad id no label has; log-probabilities are a launch of their own, made only when somebody fetches them.  Nothing
reads the device from the host, so a training step over graph-safe encoders is captured as a HIP graph."""
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

from .. import autodiff as F
from .. import ops
from .. import tf_shim
from ..checking import check_argument_types
from ..model.model_part import FeedDict, InitializerSpecs, ModelPart
from ..model.sequence import cached_index
from ..model.stateful import Stateful
from ..nn import mlp
from ..runtime import Placeholder, tensor
from ..vocabulary import Vocabulary
from .decoder import TrainResult

NO_PAD = -1           # no label is padding: ops.label_rows counts every row


class SentenceHead(ModelPart):
    """What Classifier and SequenceRegressor share: the concatenated ``output`` of the encoders as the leaves of a
    tape, the trainer's interface (``_train_loop`` / ``backward`` / ``train_loop_result``) and the hand-over of the
    encoders' gradients."""
    encoders: List[Stateful]
    targets_placeholder: Placeholder

    @property
    def input_dimension(self) -> int:
        return sum(enc.output_size for enc in self.encoders)

    def graph_safe_training(self, train_mode: bool) -> bool:
        return all(getattr(e, "graph_safe_training", lambda t: False)(train_mode) for e in self.encoders)

    def has_targets(self, ctx) -> bool:
        return ctx.is_fed(self.targets_placeholder)

    def stage_inputs(self, ctx) -> None:
        if self.has_targets(ctx):
            self.train_targets(ctx)

    def _leaves(self, tape: F.Tape, ctx):
        leaves = []
        for enc in self.encoders:
            out = enc.output(ctx)                                   # [B, output_size]
            if out.dim() != 2 or out.shape[1] != enc.output_size:
                raise ValueError("{} '{}': the output of encoder '{}' has shape {}, expected [batch, {}]".format(
                    type(self).__name__, self.name, enc, tuple(out.shape), enc.output_size))
            leaves.append(tape.leaf(out, needs_grad=True))
        if len({leaf.shape[0] for leaf in leaves}) != 1:
            raise ValueError("{} '{}': the encoders' outputs differ in batch size: {}".format(
                type(self).__name__, self.name, [tuple(leaf.shape) for leaf in leaves]))
        return leaves

    def _forward(self, ctx, want_grad: bool, grad_scale: Optional[torch.Tensor], tag: str, with_loss: bool):
        raise NotImplementedError

    # -- the interface GenericTrainer._objective_gradients calls ----------------------------------------
    def _train_loop(self, ctx, want_grad: bool = False, grad_scale: Optional[torch.Tensor] = None) -> TrainResult:
        return self._forward(ctx, want_grad, grad_scale, "head_train", True)

    def backward(self, ctx, res: TrainResult) -> None:
        sv = res.saved
        sv["tape"].backward()
        for enc, var in zip(self.encoders, sv["leaves"]):
            if var.grad is not None:
                ctx.defer_backward(enc, None, var.grad)

    @tensor
    def train_loop_result(self, ctx) -> TrainResult:
        return self._train_loop(ctx)

    @tensor
    def _inference(self, ctx) -> TrainResult:
        """The pass without targets, or beside a training pass whose outputs became their gradient."""
        key = self.train_loop_result.key
        if key in ctx.memo and not ctx.memo[key].saved["consumed"]:
            return ctx.memo[key]
        if self.has_targets(ctx) and key not in ctx.memo:
            return self.train_loop_result(ctx)
        return self._forward(ctx, False, None, "head_run", False)

    @tensor
    def cost(self, ctx):
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


class Classifier(SentenceHead):
    """Sentence classification: dense layers of the sizes ``layers`` over the concatenated ``output`` of ``encoders``,
    then one layer of the size of ``vocabulary``; behaves like a decoder that emits exactly one symbol."""

    # pylint: disable=too-many-arguments
    def __init__(self,
                 name: str,
                 encoders: List[Stateful],
                 vocabulary: Vocabulary,
                 data_id: str,
                 layers: List[int],
                 activation_fn: Callable = tf_shim.nn.relu,
                 dropout_keep_prob: float = 0.5,
                 reuse: ModelPart = None,
                 save_checkpoint: str = None,
                 load_checkpoint: str = None,
                 initializers: InitializerSpecs = None) -> None:
        """``data_id``: the series whose first token is the class; ``activation_fn`` and ``dropout_keep_prob`` apply
        after every hidden layer."""
        check_argument_types()
        ModelPart.__init__(self, name, reuse, save_checkpoint, load_checkpoint, initializers)

        self.encoders = encoders
        self.vocabulary = vocabulary
        self.data_id = data_id
        self.layers = layers
        self.activation_fn = activation_fn
        self.dropout_keep_prob = dropout_keep_prob
        self.max_output_len = 1
        self.targets_placeholder = Placeholder("{}/targets".format(name))
        if layers and mlp.activation_name(activation_fn) not in mlp.ACTIVATIONS:
            raise NotImplementedError("Classifier '{}': activation {!r} is none of tf.nn.relu, tf.tanh, tf.identity"
                                      .format(name, activation_fn))
    # pylint: enable=too-many-arguments

    DEEP = "multilayer_perceptron/deep_output_mlp"
    TOP = "multilayer_perceptron/classification_layer"

    @property
    def input_types(self) -> Dict[str, type]:
        return {self.data_id: str}

    @property
    def input_shapes(self) -> Dict[str, List]:
        return {self.data_id: [None]}

    def declare_variables(self, store) -> None:
        width = mlp.declare_multilayer_projection(self, store, self.DEEP, self.input_dimension, self.layers)
        mlp.declare_dense(self, store, self.TOP, width, len(self.vocabulary))

    # -- fed data ----------------------------------------------------------------------------------
    def feed_dict(self, dataset, train: bool = False) -> FeedDict:
        """The first token of every target sentence (pad_batch(sentences, 1), :134-143), as indices."""
        fd = ModelPart.feed_dict(self, dataset, train)
        if dataset.maybe_get_series(self.data_id) is not None:
            ids = cached_index(dataset, self.data_id, self.vocabulary, self.max_output_len, False, False)
            fd[self.targets_placeholder] = np.ascontiguousarray(ids[:, 0]) if ids.shape[1] else np.zeros(
                len(ids), np.int32)
        return fd

    @tensor
    def train_targets(self, ctx) -> torch.Tensor:
        """gt_inputs: [B] int32 on the device."""
        sess = ctx.session
        return sess.staged((id(self), "class_targets"), sess.to_device(ctx.fed(self.targets_placeholder), torch.int32,
                                                                       "class_targets"))

    def train_token_count(self, ctx) -> float:
        """Denominator of the cost: tf.reduce_mean over the batch."""
        return float(len(ctx.fed(self.targets_placeholder)))

    # -- forward -------------------------------------------------------------------------------------
    def _forward(self, ctx, want_grad: bool, grad_scale: Optional[torch.Tensor], tag: str, with_loss: bool):
        train = bool(ctx.fed(self.train_mode))
        tape = F.Tape(ctx, (id(self), tag), recording=want_grad)
        leaves = self._leaves(tape, ctx)
        bsz = leaves[0].shape[0]
        targets = None
        if with_loss:
            targets = self.train_targets(ctx)
            if tuple(targets.shape) != (bsz,):
                raise ValueError("Classifier '{}': {} targets '{}' for a batch of {}".format(
                    self.name, tuple(targets.shape), self.data_id, bsz))
        hidden = mlp.multilayer_projection(tape, ctx, self, self.DEEP, F.concat(tape, leaves), self.layers,
                                           mlp.activation_name(self.activation_fn), self.dropout_keep_prob, train)
        logits = mlp.dense(tape, self, self.TOP, hidden)             # [B, K]
        consumed = want_grad and with_loss
        saved = {"tape": tape, "leaves": leaves, "bsz": bsz, "logits": logits.data, "consumed": consumed}
        argmax = None
        if not want_grad:            # a training step wants loss and gradient only
            argmax = saved["argmax"] = ctx.buffer((id(self), tag, "argmax", bsz), (bsz,), torch.int32)
        loss_rows = F.label_xent(tape, logits, targets, NO_PAD, grad_scale, None, argmax)
        loss_sum, count = None, 0.0
        if with_loss:
            saved["loss_rows"] = loss_rows
            loss_sum = ctx.buffer((id(self), tag, "loss_sum"), (1,))
            ops.reduce_sum(loss_rows, loss_sum)
            count = self.train_token_count(ctx)
        return TrainResult(loss_sum, count, 1, saved)

    # -- fetchable surface (the reference's @tensor names) ------------------------------------------------
    @tensor
    def decoded_seq(self, ctx) -> torch.Tensor:
        """[1,B] int32: tf.argmax(logits, 1), the first maximum."""
        sv = self._inference(ctx).saved
        return sv["argmax"].view(1, sv["bsz"])

    @property
    def decoded_symbols(self):
        return self.decoded_seq

    @property
    def decoded(self):
        return self.decoded_seq

    @tensor
    def decoded_logits(self, ctx) -> torch.Tensor:
        sv = self._inference(ctx).saved
        return sv["logits"].view(1, sv["bsz"], -1)

    @tensor
    def runtime_logprobs(self, ctx) -> torch.Tensor:
        """[1,B,K] tf.nn.log_softmax(logits): a call of its own, made only when somebody fetches it."""
        logits = self.decoded_logits(ctx)
        _, bsz, k = logits.shape
        out = ctx.buffer((id(self), "logprobs", bsz, k), (bsz, k))
        ops.label_rows(logits.view(bsz, k), logprobs=out)
        return out.view(1, bsz, k)

    @property
    def loss_with_gt_ins(self):
        return self.cost

    @property
    def loss_with_decoded_ins(self):
        return self.cost
