"""Attention supervised by a reference word alignment (mirror of neuralmonkey/decoders/word_alignment_decoder.py).

``train_loss`` = sum(softmax_cross_entropy_with_logits(labels = transpose(ref_alignment, [1, 0, 2]), logits = H) *
decoder.train_padding) with H = stack(attention.histories["<decoder.name>_train"]), [T, B, S] (:100-108); ``decoded`` =
transpose(softmax(stack(histories["<decoder.name>_run"])), [1, 0, 2]), [B, T, S], and ``runtime_loss`` = 0 (:91-98).  The
histories hold the attention WEIGHTS (attention/feed_forward.py:189), so both softmaxes are taken over weights, padded
source positions (weight 0, exp(0) = 1) included: what the reference's lines say.  The part has no variables.

Three things the reference leaves open are decided here: ``Decoder.get_attention_object`` (called at :88,
defined nowhere); the fed alignment [B, max_output_len, max_length] against histories of the batch's own T and S -- row
(t, b) uses ``target[b, t, :S]``, read in place; and the gradient, which is the one TensorFlow 1.12 registers for the op,
``pad * (softmax(H) - labels)`` whatever the labels sum to.

MI355X mapping: loss rows and gradient are one launch of csrc/nm_align.hip (a wavefront per (t, b) row).  In a training
step the part computes nothing by itself: ``attach`` hangs an ``AlignmentTerm`` on the parent decoder's pass, whose
attention backward calls it between the product that writes the weights' gradient and the softmax's backward
(``Attention.backward`` on the hand-scheduled path, the steps' closures of ``AttentionTapeSession`` on the tape)."""
from typing import Dict, List, Optional

import numpy as np
import torch

from .. import ops
from ..attention.feed_forward import Attention
from ..checking import check_argument_types
from ..encoders.recurrent import RecurrentEncoder
from ..model.model_part import FeedDict, InitializerSpecs, ModelPart
from ..model.sequence import Sequence
from ..runtime import Placeholder, tensor
from .decoder import Decoder, TrainResult


def warn(message: str) -> None:
    """neuralmonkey.logging.warn."""
    import warnings
    warnings.warn(message)


class AlignmentTerm:
    """The alignment loss of one run, as the parent decoder's pass sees it: ``begin`` once the weights' shape is known
    (every check, before any launch), ``rows`` for all steps or for one, ``finish`` for the sum of the rows."""

    def __init__(self, owner: "WordAlignmentDecoder", ctx, scale: Optional[torch.Tensor]) -> None:
        self.owner, self.scale = owner, scale
        self.attention = owner.attention
        self.target = owner.alignment_on_device(ctx)               # [B, max_output_len, max_length], as fed
        self.loss_sum = ctx.buffer((id(owner), "align_loss_sum"), (1,))
        self.loss_rows = self.pad = None
        self.steps = 0

    def begin(self, ctx, weights: torch.Tensor, pad: torch.Tensor) -> None:
        steps, bsz, slen = weights.shape
        fed = tuple(self.target.shape)
        if fed[0] != bsz or steps > fed[1] or slen > fed[2]:
            raise ValueError("WordAlignmentDecoder '{}': the attention weights are [T = {}, B = {}, S = {}], the fed "
                             "alignment '{}' is [B = {}, max_output_len = {}, max_length = {}]"
                             .format(self.owner.name, steps, bsz, slen, self.owner.data_id, *fed))
        self.pad, self.steps = pad, steps
        self.loss_rows = ctx.buffer((id(self.owner), "align_loss_rows", steps, bsz), (steps, bsz))

    def rows(self, weights: torch.Tensor, first: int, dw: Optional[torch.Tensor] = None,
             accumulate: bool = False) -> None:
        """Steps ``first`` .. ``first + len(weights)``: their loss rows and, with ``dw``, their gradient."""
        last = first + weights.shape[0]
        ops.align_xent(weights, self.target[:, first:], self.pad[first:last], self.loss_rows[first:last], self.scale,
                       dw=dw, accumulate=accumulate)

    def finish(self) -> None:
        ops.reduce_sum(self.loss_rows.view(-1), self.loss_sum)

    def result(self) -> TrainResult:
        return TrainResult(self.loss_sum, 1.0, self.steps, {"term": self, "loss_rows": self.loss_rows, "dlogits": None})


class WordAlignmentDecoder(ModelPart):
    """A decoder that computes soft alignment from an attentive encoder.

    Loss is computed as cross-entropy against a reference alignment."""

    def __init__(self,
                 encoder: RecurrentEncoder,
                 decoder: Decoder,
                 data_id: str,
                 name: str,
                 reuse: ModelPart = None,
                 initializers: InitializerSpecs = None) -> None:
        check_argument_types()
        ModelPart.__init__(self, name, reuse, None, None, initializers)

        self.encoder = encoder
        self.decoder = decoder
        self.data_id = data_id
        self.ref_alignment = Placeholder("{}/{}".format(name, data_id))
        self.attention = decoder.get_attention_object(encoder, True)        # ValueError: none, or more than one
        if not isinstance(self.attention, Attention) or getattr(self.attention, "tape_only", False):
            raise TypeError("WordAlignmentDecoder '{}': the attention '{}' of decoder '{}' over encoder '{}' is a {}; "
                            "only attention.feed_forward.Attention records [T, B, S] weights that can be supervised"
                            .format(name, self.attention.name, decoder.name, encoder.name,
                                    type(self.attention).__name__))

    @property
    def dependencies(self) -> List[str]:
        # (the parent decoder has to be fed and to own variables also where no objective or runner names it)
        return ModelPart.dependencies.fget(self) + ["decoder"]

    @property
    def enc_input(self) -> Sequence:
        if not isinstance(self.encoder.input_sequence, Sequence):
            raise TypeError("Expected Sequence type in encoder.input_sequence")
        return self.encoder.input_sequence

    @property
    def input_types(self) -> Dict[str, type]:
        return {self.data_id: float}

    @property
    def input_shapes(self) -> Dict[str, List]:
        return {self.data_id: [None, self.decoder.max_output_len, self.enc_input.max_length]}

    # -- fed data --------------------------------------------------------------------------------------------------------
    def feed_dict(self, dataset, train: bool = False) -> FeedDict:
        fd = ModelPart.feed_dict(self, dataset, train)
        alignment = dataset.maybe_get_series(self.data_id)
        if alignment is None:
            if train:
                warn("Training alignment not present!")
            alignment = np.zeros((len(dataset), self.decoder.max_output_len, self.enc_input.max_length), np.float32)
        else:
            # memoised on the batch object, like the id arrays (model/sequence.py:cached_index): a batch that is executed
            # again hands back the same array, which stays resident on the device
            cache = dataset.__dict__.setdefault("_index_cache", {})
            key = (self.data_id, "alignment")
            if key not in cache:
                cache[key] = np.asarray(list(alignment), np.float32)
            alignment = cache[key]
        fd[self.ref_alignment] = alignment
        return fd

    def _fed_alignment(self, ctx) -> np.ndarray:
        """The fed array, which TensorFlow would refuse in any shape but the placeholder's."""
        fed = ctx.fed(self.ref_alignment)
        want = (int(ctx.fed(self.batch_size)), self.decoder.max_output_len, self.enc_input.max_length)
        if tuple(np.shape(fed)) != want:
            raise ValueError("WordAlignmentDecoder '{}': the fed alignment '{}' has shape {}, [batch, max_output_len, "
                             "max_length] = {} is expected".format(self.name, self.data_id, tuple(np.shape(fed)), want))
        return fed

    def alignment_on_device(self, ctx) -> torch.Tensor:
        key = (id(self), "ref_alignment")
        if key not in ctx.memo:
            fed = self._fed_alignment(ctx)                              # (the shape check, before the device is touched)
            sess = ctx.session
            ctx.memo[key] = sess.staged(key, sess.to_device(fed, torch.float32, "ref_alignment"))
        return ctx.memo[key]

    def stage_inputs(self, ctx) -> None:
        """On every training step, before a captured step is replayed: the shape check and the copy to the device."""
        if ctx.is_fed(self.ref_alignment):
            self.alignment_on_device(ctx)

    # -- the interface GenericTrainer._objective_gradients calls ------------------------------------------------------------
    # The cost is a plain sum over the batch (:108), like CTCDecoder's: the gradient scale is the objective's weight on
    # every rank and nothing is divided by a token count.
    loss_is_batch_sum = True

    def train_token_count(self, ctx) -> float:
        return self.decoder.train_token_count(ctx)

    def graph_safe_training(self, train_mode: bool) -> bool:
        """The parent's: the kernel reads no size on the host and takes its scale from a device scalar."""
        return self.decoder.graph_safe_training(train_mode)

    def attach(self, ctx, scale: torch.Tensor, parent_trained: bool) -> None:
        """Hang this objective's term on the parent decoder's pass of the run ``ctx``.  ``parent_trained``: the parent is
        an objective of the same trainer and runs its forward + backward itself; otherwise ``_train_loop`` / ``backward``
        below run them, with a zero cross-entropy scale."""
        term = AlignmentTerm(self, ctx, scale)
        ctx.memo.setdefault((id(self.decoder), "alignment_terms"), []).append(term)
        ctx.memo[(id(self), "alignment_term")] = (term, parent_trained)
        if not parent_trained:
            ctx.buffer((id(self), "zero_scale"), (1,), zero=True)

    def _train_loop(self, ctx, want_grad: bool = False, grad_scale: Optional[torch.Tensor] = None) -> TrainResult:
        attached = ctx.memo.get((id(self), "alignment_term"))
        if attached is None:                                          # no trainer: the loss of the parent's own pass
            return self._loss_of_recorded_weights(ctx)
        term, parent_trained = attached
        parent = None
        if not parent_trained:
            zero = ctx.buffer((id(self), "zero_scale"), (1,))
            # (always with a backward pass: the term's launch is part of it)
            parent = self.decoder._train_loop(ctx, want_grad=True, grad_scale=zero)   # pylint: disable=protected-access
        elif term.loss_rows is None:
            raise RuntimeError("WordAlignmentDecoder '{}': the pass of its decoder '{}' has not run"
                               .format(self.name, self.decoder.name))
        res = term.result()
        if parent is not None:
            res.saved["parent"] = parent
        return res

    def backward(self, ctx, res: TrainResult) -> None:
        if "parent" in res.saved:
            self.decoder.backward(ctx, res.saved["parent"])

    def _loss_of_recorded_weights(self, ctx) -> TrainResult:
        self.decoder.train_loop_result(ctx)
        term = AlignmentTerm(self, ctx, None)
        weights = self.attention.histories["{}_train".format(self.decoder.name)]
        term.begin(ctx, weights, self.decoder.train_mask(ctx))
        term.rows(weights, 0)
        term.finish()
        return term.result()

    # -- fetchable surface (the reference's @tensor names) ----------------------------------------------------------------
    @tensor
    def train_loop_result(self, ctx) -> TrainResult:
        return self._train_loop(ctx)

    @tensor
    def train_loss(self, ctx):
        return self.train_loop_result(ctx).loss_sum[0]

    @property
    def cost(self):
        return self.train_loss

    @tensor
    def train_xents(self, ctx) -> torch.Tensor:
        """[T, B]: xent * train_padding before the reduce_sum."""
        return self.train_loop_result(ctx).saved["loss_rows"]

    @tensor
    def decoded(self, ctx) -> torch.Tensor:
        """[B, T, S]: the softmax of the weights the runtime loop recorded, batch-major."""
        self.decoder.runtime_loop_result(ctx)
        weights = self.attention.histories["{}_run".format(self.decoder.name)]
        steps, bsz, slen = weights.shape
        out = ctx.buffer((id(self), "decoded", bsz, steps, slen), (bsz, steps, slen))
        return ops.align_softmax(weights, out)

    @tensor
    def runtime_loss(self, ctx):
        return 0
