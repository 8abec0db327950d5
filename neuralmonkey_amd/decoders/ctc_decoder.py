"""Connectionist temporal classification head (mirror of neuralmonkey/decoders/ctc_decoder.py).

``logits`` = encoder.temporal_states [B,T,D] . state_to_word_W [D, V+1] + state_to_word_b (:110-140; the blank is the
LAST class, index V = len(vocabulary), as tf.nn.ctc_loss numbers it); ``cost`` = tf.reduce_sum(tf.nn.ctc_loss(...,
ignore_longer_outputs_than_inputs=True)) over the frames below each sentence's encoder length (:99-108) -- a plain sum,
not divided by anything; ``decoded`` = tf.nn.ctc_greedy_decoder, densified with END_TOKEN_INDEX and time-major (:75-89),
which is what PlainRunner hands to ``vectors_to_sentences``.

MI355X mapping: the product is the fp32 MFMA GEMM with its bias epilogue over the batch-major rows [B*T, D]; the CTC
kernels read those rows as [T, B, V+1] through strides (no transposed copy).  Loss, gradient and greedy decoding are
csrc/nm_ctc.hip: row log-sum-exps, the alpha and beta recursions of a sentence side by side in two workgroups, a
row-parallel gradient pass that overwrites the logits (scaled by the trainer's device-side ``grad_scale``), and a
ballot compaction of the frames' argmax classes -- only int32 tokens cross to the host.  Label preparation (pad
removal, ``merge_repeated_targets``) happens on the host at feed time, like every other id lookup of this engine.
"""
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import autodiff as F
from .. import ops
from ..checking import check_argument_types
from ..model.model_part import FeedDict, InitializerSpecs, ModelPart
from ..model.sequence import cached_index
from ..model.stateful import TemporalStateful
from ..runtime import Placeholder, tensor
from ..variables import zeros_initializer
from ..vocabulary import END_TOKEN_INDEX, PAD_TOKEN_INDEX, Vocabulary
from .decoder import TrainResult


def uniform_initializer(low: float, high: float):
    """tf.random_uniform_initializer(low, high)."""
    def init(rng, shape):
        return rng.uniform(low, high, size=shape).astype(np.float32)
    return init


def prepare_labels(ids: np.ndarray, merge_repeated: bool) -> Tuple[np.ndarray, np.ndarray]:
    """Padded target ids [B, L] -> (labels [B, L'] int32, lengths [B] int32) as tf.nn.ctc_loss sees them: <pad>
    positions removed (the SparseTensor of ctc_decoder.py:63-73) and, with ``merge_repeated``
    (preprocess_collapse_repeated), adjacent equal labels collapsed into one."""
    ids = np.asarray(ids, dtype=np.int32).reshape(len(ids), -1)
    rows = []
    for row in ids:
        kept = row[row != PAD_TOKEN_INDEX]
        if merge_repeated and kept.size > 1:
            kept = kept[np.concatenate(([True], kept[1:] != kept[:-1]))]
        rows.append(kept)
    lengths = np.asarray([r.size for r in rows], dtype=np.int32)
    labels = np.zeros((len(rows), int(lengths.max()) if len(rows) else 0), dtype=np.int32)
    for i, r in enumerate(rows):
        labels[i, :r.size] = r
    return labels, lengths


class CTCDecoder(ModelPart):
    # pylint: disable=too-many-arguments
    def __init__(self,
                 name: str,
                 encoder: TemporalStateful,
                 vocabulary: Vocabulary,
                 data_id: str,
                 max_length: int = None,
                 merge_repeated_targets: bool = False,
                 merge_repeated_outputs: bool = True,
                 beam_width: int = 1,
                 reuse: ModelPart = None,
                 save_checkpoint: str = None,
                 load_checkpoint: str = None,
                 initializers: InitializerSpecs = None) -> None:
        check_argument_types()
        ModelPart.__init__(self, name, reuse, save_checkpoint, load_checkpoint, initializers)

        self.encoder = encoder
        self.vocabulary = vocabulary
        self.data_id = data_id
        self.max_length = max_length

        self.merge_repeated_targets = merge_repeated_targets
        self.merge_repeated_outputs = merge_repeated_outputs
        self.beam_width = beam_width
        self.train_tokens = Placeholder("{}/target_tokens".format(name))
    # pylint: enable=too-many-arguments

    @property
    def input_types(self) -> Dict[str, type]:
        return {self.data_id: str}

    @property
    def input_shapes(self) -> Dict[str, List]:
        return {self.data_id: [None, None]}

    def graph_safe_training(self, train_mode: bool) -> bool:
        return False          # the emitted width of ``decoded`` is read on the host; CTC inside a step graph is out of scope

    def declare_variables(self, store) -> None:
        classes = len(self.vocabulary) + 1
        self.declare(store, "state_to_word_W", (self.encoder.dimension, classes), uniform_initializer(-0.5, 0.5))
        self.declare(store, "state_to_word_b", (classes,), zeros_initializer())

    # -- fed data ----------------------------------------------------------------------------------
    def feed_dict(self, dataset, train: bool = False) -> FeedDict:
        fd = ModelPart.feed_dict(self, dataset, train)
        sentences = dataset.maybe_get_series(self.data_id)
        if sentences is None and train:
            raise ValueError("You must feed reference sentences when training")
        if sentences is not None:
            fd[self.train_tokens] = cached_index(dataset, self.data_id, self.vocabulary, self.max_length, False, False)
        return fd

    def has_targets(self, ctx) -> bool:
        return ctx.is_fed(self.train_tokens)

    def _prepared(self, ctx) -> Tuple[np.ndarray, np.ndarray]:
        """(labels, lengths) of the fed batch, memoised on the fed array: a batch that is executed again hands back the
        same arrays, which keeps them resident on the device (Session.to_device caches by identity)."""
        ids = ctx.fed(self.train_tokens)
        cache = self.__dict__.setdefault("_label_cache", {})
        hit = cache.get(id(ids))
        if hit is None or hit[0] is not ids:
            if len(cache) > 64:
                cache.clear()
            hit = cache[id(ids)] = (ids,) + prepare_labels(ids, self.merge_repeated_targets)
        return hit[1], hit[2]

    @tensor
    def train_targets(self, ctx) -> Tuple[torch.Tensor, torch.Tensor]:
        """(labels [B, L'] int32, label lengths [B] int32) on the device."""
        labels, lengths = self._prepared(ctx)
        sess = ctx.session
        return (sess.staged((id(self), "ctc_labels"), sess.to_device(labels, torch.int32, "ctc_labels")),
                sess.staged((id(self), "ctc_label_len"), sess.to_device(lengths, torch.int32, "ctc_label_len")))

    def stage_inputs(self, ctx) -> None:
        if self.has_targets(ctx):
            self.train_targets(ctx)

    @tensor
    def frame_lengths(self, ctx) -> torch.Tensor:
        """encoder.lengths (model/stateful.py:55-62): int32 row sums of the encoder's temporal mask."""
        mask = self.encoder.temporal_mask(ctx)
        out = ctx.buffer((id(self), "frame_len", mask.shape[0]), (mask.shape[0],), torch.int32)
        return ops.ctc_mask_lengths(mask, out)

    # -- the interface GenericTrainer._objective_gradients calls ----------------------------------------
    # The cost is a plain sum over the sentences, not a mean over target tokens.  GenericTrainer._objective_gradients
    # reads this: the gradient scale is the objective's weight on every rank, with no count summed over the ranks
    # (that sum, 1 per rank, would divide the gradient by the number of ranks).  Under data parallelism every rank
    # back-propagates its own sentences' sum, the gradient exchange adds the ranks' gradients up to the gradient of the
    # full batch's sum, and a fetched ``cost`` is the RANK'S OWN sum (the full batch's cost is the sum over ranks).
    loss_is_batch_sum = True

    def train_token_count(self, ctx) -> float:
        """The cost is a plain sum over the batch: the trainer's ``weight / count`` scale is the objective's weight."""
        return 1.0

    def _forward(self, ctx, want_grad: bool, grad_scale: Optional[torch.Tensor], tag: str, with_loss: bool):
        tape = F.Tape(ctx, (id(self), tag), recording=want_grad)
        states = self.encoder.temporal_states(ctx)                         # [B,T,D]
        bsz, steps, dim = states.shape
        x = tape.leaf(states.reshape(bsz * steps, dim), needs_grad=True)
        logits = F.linear(tape, x, tape.param(self, "state_to_word_W"), tape.param(self, "state_to_word_b"))
        saved = {"tape": tape, "x": x, "bsz": bsz, "steps": steps, "dim": dim, "logits": logits.data,
                 "dlogits": logits.data if want_grad else None}
        loss_sum = None
        if with_loss:
            labels, label_len = self.train_targets(ctx)
            loss, loss_sum = F.ctc_loss(tape, logits, bsz, steps, labels, label_len, self.frame_lengths(ctx),
                                        self.merge_repeated_outputs, grad_scale)
            saved["loss_rows"] = loss
        return TrainResult(loss_sum, 1.0, steps, saved)

    def _train_loop(self, ctx, want_grad: bool = False, grad_scale: Optional[torch.Tensor] = None) -> TrainResult:
        return self._forward(ctx, want_grad, grad_scale, "ctc_train", True)

    def backward(self, ctx, res: TrainResult) -> None:
        sv = res.saved
        sv["tape"].backward()
        if sv["x"].grad is not None:
            ctx.defer_backward(self.encoder, sv["x"].grad.view(sv["bsz"], sv["steps"], sv["dim"]), None)

    # -- fetchable surface (the reference's @tensor names) ------------------------------------------------
    @tensor
    def train_loop_result(self, ctx) -> TrainResult:
        return self._train_loop(ctx)

    @tensor
    def _inference(self, ctx) -> TrainResult:
        """The product alone, for runs that feed no targets."""
        key = self.train_loop_result.key
        if key in ctx.memo and ctx.memo[key].saved["dlogits"] is None:
            return ctx.memo[key]
        return self._forward(ctx, False, None, "ctc_run", False)

    @tensor
    def logits(self, ctx) -> torch.Tensor:
        """[T, B, V+1], time-major (:140) -- a strided view of the batch-major product."""
        sv = (self.train_loop_result(ctx) if self.has_targets(ctx) else self._inference(ctx)).saved
        if sv["dlogits"] is not None:
            sv = self._inference(ctx).saved           # the training pass overwrote its logits with their gradient
        return sv["logits"].view(sv["bsz"], sv["steps"], -1).transpose(0, 1)

    @tensor
    def cost(self, ctx):
        if not self.has_targets(ctx):
            return 0.0
        return self.train_loop_result(ctx).loss_sum[0]

    @property
    def train_loss(self):
        return self.cost

    @property
    def runtime_loss(self):
        return self.cost

    @tensor
    def sentence_losses(self, ctx) -> torch.Tensor:
        """[B]: tf.nn.ctc_loss before the reduce_sum (0 for a sentence without a valid alignment)."""
        return self.train_loop_result(ctx).saved["loss_rows"]

    @tensor
    def decoded(self, ctx) -> torch.Tensor:
        """[max(1, longest emitted sequence), B] int32, padded with END_TOKEN_INDEX (a batch that emits nothing keeps
        one all-END row, from which ``vectors_to_sentences`` reads the batch size and empty sentences)."""
        if self.beam_width != 1:
            raise NotImplementedError("CTCDecoder '{}': beam_width = {} needs tf.nn.ctc_beam_search_decoder, which this "
                                      "engine does not implement (greedy decoding only: beam_width = 1)"
                                      .format(self.name, self.beam_width))
        logits = self.logits(ctx)
        steps, bsz, _ = logits.shape
        if steps == 0:
            return np.full((1, bsz), END_TOKEN_INDEX, dtype=np.int32)
        tokens = ctx.buffer((id(self), "ctc_tokens", bsz, steps), (bsz, steps), torch.int32)
        out_len = ctx.buffer((id(self), "ctc_out_len", bsz), (bsz,), torch.int32)
        ops.ctc_greedy(logits, self.frame_lengths(ctx), self.merge_repeated_outputs, END_TOKEN_INDEX, tokens, out_len)
        width = max(1, int(np.max(ctx.session.read_small(out_len), initial=0)))      # B int32 words to the host
        return tokens[:, :width].t()
