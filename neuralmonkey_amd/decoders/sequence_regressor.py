"""``SequenceRegressor``: an MLP regression over the encoders' ``output`` vectors (mirror of
neuralmonkey/decoders/sequence_regressor.py).

``predictions`` [B, dimension] = output_projection(mlp(concat(outputs))); the target is the first value of each row of
the data series and broadcasts over the dimension; ``cost`` = mean over B * dimension of (prediction - target)^2.

MI355X mapping: the layers are the fp32 MFMA GEMM; the squared error of a row and its gradient in place (scaled by the
trainer's device-side ``grad_scale`` = weight / (B * dimension)) are one launch of csrc/nm_pool.hip."""
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

from .. import autodiff as F
from .. import ops
from .. import tf_shim
from ..checking import check_argument_types
from ..model.model_part import FeedDict, InitializerSpecs, ModelPart
from ..model.stateful import Stateful
from ..nn import mlp
from ..runtime import Placeholder, tensor
from .classifier import SentenceHead
from .decoder import TrainResult


class SequenceRegressor(SentenceHead):
    """Sentence regression: dense layers of the sizes ``layers`` over the concatenated ``output`` of ``encoders``, then
    ``output_projection`` to ``dimension`` values, trained on the squared error against the first value of a row."""

    # pylint: disable=too-many-arguments
    def __init__(self,
                 name: str,
                 encoders: List[Stateful],
                 data_id: str,
                 layers: List[int] = None,
                 activation_fn: Callable = tf_shim.nn.relu,
                 dropout_keep_prob: float = 1.0,
                 dimension: int = 1,
                 reuse: ModelPart = None,
                 save_checkpoint: str = None,
                 load_checkpoint: str = None,
                 initializers: InitializerSpecs = None) -> None:
        check_argument_types()
        ModelPart.__init__(self, name, reuse, save_checkpoint, load_checkpoint, initializers)

        self.encoders = encoders
        self.data_id = data_id
        self.max_output_len = 1
        self.dimension = dimension

        self._layers = layers
        self._activation_fn = activation_fn
        self._dropout_keep_prob = dropout_keep_prob
        self.targets_placeholder = Placeholder("{}/targets".format(name))
        if layers and mlp.activation_name(activation_fn) not in mlp.ACTIVATIONS:
            raise NotImplementedError("SequenceRegressor '{}': activation {!r} is none of tf.nn.relu, tf.tanh, "
                                      "tf.identity".format(name, activation_fn))
    # pylint: enable=too-many-arguments

    MLP = "mlp"
    TOP = "output_projection"

    @property
    def layer_sizes(self) -> List[int]:
        """(the reference iterates over ``layers`` as given: None, its default, fails there; it means no layers here)"""
        return list(self._layers or [])

    @property
    def input_types(self) -> Dict[str, type]:
        return {self.data_id: float}

    @property
    def input_shapes(self) -> Dict[str, List]:
        return {self.data_id: [None]}

    def declare_variables(self, store) -> None:
        width = mlp.declare_multilayer_projection(self, store, self.MLP, self.input_dimension, self.layer_sizes)
        mlp.declare_dense(self, store, self.TOP, width, self.dimension)

    # -- fed data ----------------------------------------------------------------------------------
    def feed_dict(self, dataset, train: bool = False) -> FeedDict:
        """The first value of every row of the series (:98-106)."""
        fd = ModelPart.feed_dict(self, dataset, train)
        sentences = dataset.maybe_get_series(self.data_id)
        if sentences is not None:
            cache = dataset.__dict__.setdefault("_index_cache", {})
            key = (self.data_id, "first_value")
            if key not in cache:
                cache[key] = np.asarray([row[0] for row in list(sentences)], dtype=np.float32)
            fd[self.targets_placeholder] = cache[key]
        return fd

    @tensor
    def train_targets(self, ctx) -> torch.Tensor:
        """train_inputs: [B] float32 on the device."""
        sess = ctx.session
        return sess.staged((id(self), "regression_targets"),
                           sess.to_device(ctx.fed(self.targets_placeholder), torch.float32, "regression_targets"))

    def train_token_count(self, ctx) -> float:
        """Denominator of the cost: tf.reduce_mean over batch and dimension."""
        return float(len(ctx.fed(self.targets_placeholder)) * self.dimension)

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
                raise ValueError("SequenceRegressor '{}': {} targets '{}' for a batch of {}".format(
                    self.name, tuple(targets.shape), self.data_id, bsz))
        hidden = mlp.multilayer_projection(tape, ctx, self, self.MLP, F.concat(tape, leaves), self.layer_sizes,
                                           mlp.activation_name(self._activation_fn), self._dropout_keep_prob, train)
        pred = mlp.dense(tape, self, self.TOP, hidden)               # [B, dimension]
        consumed = want_grad and with_loss
        saved = {"tape": tape, "leaves": leaves, "bsz": bsz, "predictions": pred.data, "consumed": consumed}
        loss_rows = F.squared_error(tape, pred, targets, grad_scale)
        loss_sum, count = None, 0.0
        if with_loss:
            saved["loss_rows"] = loss_rows
            loss_sum = ctx.buffer((id(self), tag, "loss_sum"), (1,))
            ops.reduce_sum(loss_rows, loss_sum)
            count = self.train_token_count(ctx)
        return TrainResult(loss_sum, count, 1, saved)

    # -- fetchable surface ------------------------------------------------------------------------------------
    @tensor
    def predictions(self, ctx) -> torch.Tensor:
        return self._inference(ctx).saved["predictions"]

    @property
    def decoded(self):
        return self.predictions
