"""Training objectives for reinforcement learning (mirror of neuralmonkey/trainers/rl_trainer.py): REINFORCE with
sentence-level feedback on ``sample_size`` sampled decodings.

    sent_logprob[s, b] = -sum_t nll(sampled symbol | logits / temperature)      over ALL steps of sample s's loop
    baseline           = reward_sum / max(reward_counter, 1)                     both updated BEFORE use (:149-164)
    p                  = softmax_s(alpha * sent_logprob) with ``normalize``, else sent_logprob
    loss               = mean_b sum_s -(reward[s, b] - baseline) * p[s, b]   [+ ce_smoothing * decoder.cost]

Rewards and baseline are constants of the derivative.  The sum over the steps is unmasked, as in the reference (:138-140):
the ``<pad>`` rows of sentences that have finished count.

MI355X mapping: the reference calls an evaluator object once per sentence and per sample behind ``tf.py_func`` --
``sample_size * B`` joins and splits of Python strings and a device-to-host read-back per sample.  Here a
``GLEUEvaluator`` / ``BLEUEvaluator`` over a vocabulary whose words are whole words scores all sentences of a sample in ONE
launch on token indices (``nm_eval_sentence_score``), ``nm_reinforce_sample_weights`` turns rewards, sentence
log-probabilities and the baseline's two device scalars into the row weights and the scalar of ``nm_xent`` over every
sample's taped logits, whose gradient is written in place; after the sampling loops the step reads nothing back.  Over
a vocabulary of subword PIECES (words that end with "@@") the same evaluators run in one launch too
(``nm_eval_joined_sentence_score``): a joined word is its length in bytes and two polynomial hashes composed on the
device from a per-vocabulary table (``piece_table``), so there equality of words is equality of (length, hash) -- see
include/nmhip_subword.h for the collision bound.  Any other callable gets the reference's treatment: indices to
strings, the BPE join, one call per sentence on the host.
"""
import warnings
from typing import Callable, List, Optional

import numpy as np
import torch

from .. import autodiff as F
from .. import ops
from ..checking import check_argument_types
from ..decoders.decoder import Decoder
from ..evaluators.bleu import BLEUEvaluator
from ..evaluators.gleu import GLEUEvaluator
from ..variables import zeros_initializer
from ..runtime import register_part, tensor
from ..vocabulary import END_TOKEN, END_TOKEN_INDEX, PAD_TOKEN, PAD_TOKEN_INDEX
from .objective import Objective
from .self_critical_objective import _Taped

# pylint: disable=invalid-name
RewardFunction = Callable[[np.ndarray, np.ndarray], np.ndarray]
# pylint: enable=invalid-name

# the baseline's state, under the names the reference's graph gives the two tf.Variable objects (:151-153: the
# objective is no model part, so they live in no scope)
REWARD_COUNTER, REWARD_SUM = "reward_counter", "reward_sum"


def words_are_indices(vocabulary) -> bool:
    """True when equal word sequences are equal index sequences after the reference's BPE join (:110-111,
    ``" ".join(words).replace("@@ ", "").split(" ")``): no word ends with "@@", is empty or holds a space.  Computed
    once per vocabulary."""
    cached = getattr(vocabulary, "_words_are_indices", None)
    if cached is None or cached[0] != len(vocabulary):
        words = list(vocabulary.index_to_word)
        plain = all(w and " " not in w and not w.endswith("@@") for w in words) and len(set(words)) == len(words)
        cached = (len(vocabulary), plain)
        vocabulary._words_are_indices = cached             # pylint: disable=protected-access
    return cached[1]


# the two polynomial hashes of a joined word (include/nmhip_subword.h): H(s) = sum_i (byte_i + 1) * P^(len - 1 - i) mod M
PIECE_MODULI = (2147483647, 2147483629)                  # 2^31 - 1 and 2^31 - 19, primes
PIECE_BASES = (1103515245, 1664525)
PIECE_CONTINUES, PIECE_CUTS = 1, 2                       # the flags of a table row


def _piece_element(text: str) -> tuple:
    """(hash mod M1, hash mod M2, P1^len mod M1, P2^len mod M2, len) of the UTF-8 bytes of ``text``."""
    data = text.encode("utf-8")
    out = []
    for modulus, base in zip(PIECE_MODULI, PIECE_BASES):
        value = 0
        for byte in data:
            value = (value * base + byte + 1) % modulus
        out.append(value)
    return (out[0], out[1], pow(PIECE_BASES[0], len(data), PIECE_MODULI[0]),
            pow(PIECE_BASES[1], len(data), PIECE_MODULI[1]), len(data))


def _compose(left: tuple, right: tuple) -> tuple:
    """The element of ``left`` followed by ``right``: H(s + t) = H(s) * P^len(t) + H(t)."""
    (m1, m2) = PIECE_MODULI
    return ((left[0] * right[2] + right[0]) % m1, (left[1] * right[3] + right[1]) % m2, left[2] * right[2] % m1,
            left[3] * right[3] % m2, left[4] + right[4])


def piece_table(vocabulary) -> Optional[np.ndarray]:
    """The table of ``ops.eval_joined_sentence_score``: int32 [V, 12], per entry the element of the stem (the text without
    a trailing "@@"), the element of the whole text, the flags (continuation piece, ``</s>`` or ``<pad>`` BY STRING: a
    vocabulary may repeat a word) and 0.  ``None`` for a vocabulary with an empty word or a word that holds a space, where
    the reference's join is not the rule the kernel applies.  Computed once per vocabulary."""
    cached = getattr(vocabulary, "_piece_table", None)
    if cached is None or cached[0] != len(vocabulary):
        words = list(vocabulary.index_to_word)
        table = None
        if all(w and " " not in w for w in words):
            table = np.zeros((len(words), ops.PIECE_TABLE_ROW), np.int32)
            for row, word in zip(table, words):
                continues = word.endswith("@@")
                row[0:5] = _piece_element(word[:-2] if continues else word)
                row[5:10] = _piece_element(word)
                row[10] = (PIECE_CONTINUES if continues else 0) | (PIECE_CUTS if word in (END_TOKEN, PAD_TOKEN) else 0)
        cached = (len(vocabulary), table, {})
        vocabulary._piece_table = cached                    # pylint: disable=protected-access
    return cached[1]


def device_piece_table(vocabulary, device) -> torch.Tensor:
    """``piece_table`` on ``device``, copied there once per (vocabulary, device)."""
    table = piece_table(vocabulary)
    on_devices = vocabulary._piece_table[2]                 # pylint: disable=protected-access
    key = str(torch.device(device))
    if key not in on_devices:
        on_devices[key] = torch.from_numpy(table).to(device)
    return on_devices[key]


def joined_word_keys(vocabulary, column) -> List[tuple]:
    """The keys (bytes, hash mod M1, hash mod M2) of the joined words of one column of piece indices, from the rows of
    ``piece_table`` alone -- what the kernel computes, stated on the host: the cut at the first flagged token, a
    continuation piece with a kept token behind it lends its stem to the next word, every other kept token ends a word
    with its whole text; an empty column is the one word of no bytes."""
    table = piece_table(vocabulary)
    kept = []
    for index in column:
        if not 0 <= index < len(table) or table[index][10] & PIECE_CUTS:
            break
        kept.append(int(index))
    keys, open_word = [], (0, 0, 1, 1, 0)
    for position, index in enumerate(kept):
        row = [int(v) for v in table[index]]
        if row[10] & PIECE_CONTINUES and position != len(kept) - 1:
            open_word = _compose(open_word, tuple(row[0:5]))
        else:
            done = _compose(open_word, tuple(row[5:10]))
            keys.append((done[4], done[0], done[1]))
            open_word = (0, 0, 1, 1, 0)
    return keys or [(0, 0, 0)]


def word_key(word: str) -> tuple:
    """The key of one joined word, from its characters."""
    element = _piece_element(word)
    return (element[4], element[0], element[1])


def score_on_the_host(vocabulary, reward_function, references: np.ndarray, hypotheses: np.ndarray) -> np.ndarray:
    """rl_trainer.py:83-115: time-major index arrays to one float32 reward per sentence -- the words up to the first
    ``</s>`` or ``<pad>``, the BPE join, ``reward_function([hypothesis], [reference])``."""
    words = vocabulary.index_to_word
    rewards = []
    for refs, hyps in zip(np.transpose(references), np.transpose(hypotheses)):
        sequences = []
        for column in (refs, hyps):
            kept = []
            for index in column:
                token = words[index]
                if token in (END_TOKEN, PAD_TOKEN):
                    break
                kept.append(token)
            sequences.append(" ".join(kept).replace("@@ ", "").split(" "))
        rewards.append(float(reward_function([sequences[1]], [sequences[0]])))
    return np.array(rewards, dtype=np.float32)


# pylint: disable=too-many-instance-attributes
class ReinforceObjective(Objective):
    """rl_trainer.py:22-192.  Depending on the options the objective is
    1) ``sample_size = 1, normalize = False, ce_smoothing = 0``: the bandit objective of Kreutzer et al. 2017
       (http://www.aclweb.org/anthology/P17-1138, eq. 2), best with ``subtract_baseline``;
    2) ``sample_size > 1, normalize = True, ce_smoothing = 0``: minimum risk training (Shen et al. 2016,
       http://www.aclweb.org/anthology/P16-1159, eq. 12);
    3) ``sample_size > 1, normalize = False, ce_smoothing = 0``: the REINFORCE objective of Wu et al. 2016
       (https://arxiv.org/abs/1609.08144, eq. 8);
    4) ... with ``ce_smoothing > 0``: their mixed objective (eq. 9).
    ``alpha`` sharpens the distribution over the samples, ``temperature`` the one the samples are drawn from."""
    wants_train_argmax = False           # (GenericTrainer: nothing here reads the teacher-forced pass's argmax)

    # pylint: disable=too-many-arguments
    def __init__(self, decoder: Decoder, reward_function: RewardFunction, subtract_baseline: bool = False,
                 normalize: bool = False, temperature: float = 1., ce_smoothing: float = 0., alpha: float = 1.,
                 sample_size: int = 1) -> None:
        check_argument_types()
        Objective.__init__(self, "{}_rl".format(decoder.name), decoder)
        self.reward_function = reward_function
        self.subtract_baseline = subtract_baseline
        self.normalize = normalize
        self.temperature = temperature
        self.ce_smoothing = ce_smoothing
        self.alpha = alpha
        self.sample_size = sample_size
        if sample_size < 1 or sample_size > 64:
            raise ValueError("sample_size must be between 1 and 64, got {}".format(sample_size))
        if subtract_baseline:
            register_part(self)                    # the session's store gets the baseline's two scalars
    # pylint: enable=too-many-arguments

    def declare_variables(self, store) -> None:
        for name in (REWARD_COUNTER, REWARD_SUM):
            store.declare(name, (), zeros_initializer(), trainable=False)

    # -- rewards ------------------------------------------------------------------------------------------------
    def evaluator_reward(self) -> Optional[tuple]:
        """(kind, order) when the reward is one the kernels compute: a GLEU or BLEU evaluator proper, without
        de-duplication, BLEU with one reference, orders up to 4."""
        fn = self.reward_function
        if type(fn) not in (GLEUEvaluator, BLEUEvaluator) or fn.deduplicate or not 1 <= fn.n <= 4:
            return None
        if isinstance(fn, BLEUEvaluator) and fn.multiple_references_separator is not None:
            return None
        return ("bleu" if isinstance(fn, BLEUEvaluator) else "gleu"), fn.n

    def device_reward(self) -> Optional[tuple]:
        """(kind, order) when the reward runs as ``ops.eval_sentence_score``: an evaluator of ``evaluator_reward`` over a
        vocabulary of whole words, where equal words are equal indices."""
        if not words_are_indices(self.decoder.vocabulary):
            return None
        return self.evaluator_reward()

    def joined_device_reward(self) -> Optional[tuple]:
        """(kind, order) when the reward runs as ``ops.eval_joined_sentence_score``: the same evaluators over any
        vocabulary that has a ``piece_table`` -- a BPE vocabulary, where two piece sequences can spell one word and the
        kernel compares (length, hash) of the joined words."""
        if piece_table(self.decoder.vocabulary) is None:
            return None
        return self.evaluator_reward()

    def rewards(self, ctx, references: torch.Tensor, hypotheses: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """One float32 per sentence into ``out`` [B] on the device.  The evaluators of ``device_reward`` and, over
        subword pieces, of ``joined_device_reward``: one kernel launch.  Anything else: the reference's ``tf.py_func``
        -- both arrays to the host (a synchronisation), one call per sentence, the result back."""
        on_device = self.device_reward()
        if on_device is not None and references.is_cuda:
            return ops.eval_sentence_score(on_device[0], on_device[1], references, hypotheses, END_TOKEN_INDEX,
                                           PAD_TOKEN_INDEX, out=out)
        joined = self.joined_device_reward()
        if joined is not None and references.is_cuda:
            table = device_piece_table(self.decoder.vocabulary, references.device)
            return ops.eval_joined_sentence_score(joined[0], joined[1], references, hypotheses, table, out=out)
        host = score_on_the_host(self.decoder.vocabulary, self.reward_function, references.cpu().numpy(),
                                 hypotheses.cpu().numpy().astype(np.int64))
        return out.copy_(torch.from_numpy(np.ascontiguousarray(host.reshape(out.shape))))

    # -- the term ------------------------------------------------------------------------------------------------
    # pylint: disable=too-many-locals,protected-access
    def forward_backward(self, ctx, weight: float, want_grad: bool = True, samples: Optional[torch.Tensor] = None) -> dict:
        """``sample_size`` taped sampling loops, their rewards, the loss and -- with ``want_grad`` -- its gradient: into
        the flat gradient buffer (accumulated) and, through ``ctx.defer_backward``, into the encoders.  With
        ``ce_smoothing`` the teacher-forced pass runs first (its hand-scheduled backward overwrites its slices of the
        flat gradient, the tapes add to them).

        ``samples``: int32 [S, T, B] of symbols to REPLAY instead of drawing -- a reproducibility hook (recorded draws
        of another implementation, a failing step); every loop stops by the usual rule, applied to the replayed
        symbols.

        Returns ``loss``, ``rewards`` [S, B], ``baseline``, ``sent_logprobs`` [S, B] (device tensors) and, per sample,
        ``symbols`` ([steps, B] int32), ``steps``, ``logits`` (with ``want_grad`` False: [steps, B, V], divided by the
        temperature) and the ``salts`` of the draws."""
        dec = self.decoder
        sess = ctx.session
        count_s = self.sample_size
        cost = None
        if self.ce_smoothing > 0.0:                           # :184-185, the normalisation of CostObjective
            count = dec.train_token_count(ctx)
            ce_scale = ctx.buffer((id(self), "ce_scale"), (1,))
            ops.fill(ce_scale, weight * self.ce_smoothing / count if count else 0.0)
            res = dec._train_loop(ctx, want_grad=want_grad, grad_scale=ce_scale)
            cost = ctx.buffer((id(self), "ce_cost"), (1,))
            ops.ew("scale", res.loss_sum[0:1], None, cost, alpha=self.ce_smoothing / count if count else float("nan"))
            if want_grad:
                dec.backward(ctx, res)
                sess.join_side()      # (the leaf products of that backward write their slices on side lanes)
        if samples is not None:
            bsz_fed = int(ctx.fed(dec.batch_size))
            if (samples.dim() != 3 or samples.dtype != torch.int32 or samples.shape[0] != count_s
                    or not 1 <= samples.shape[1] <= dec.max_output_len or samples.shape[2] != bsz_fed):
                raise ValueError("samples must be int32 [sample_size = {}, at most max_output_len = {} steps, batch = {}]"
                                 ", got {} {}".format(count_s, dec.max_output_len, bsz_fed, samples.dtype,
                                                      tuple(samples.shape)))
            samples = samples.to(sess.device).contiguous()
        references = dec.train_inputs(ctx)
        runs = []
        for s in range(count_s):                              # :120-126
            runs.append(dec.taped_runtime_loop(ctx, record=want_grad, sample=True, temperature=float(self.temperature),
                                               tag="sample{}".format(s),
                                               replay=None if samples is None else samples[s]))
        bsz = runs[0]["bsz"]
        tmax = max(run["enqueued"] for run in runs)
        steps = [run["steps"] for run in runs]
        key = (id(self), "term", count_s, tmax, bsz)
        reward = ctx.buffer(key + ("reward",), (count_s, bsz))
        logprob = ctx.buffer(key + ("logprob",), (count_s, bsz))
        for s, run in enumerate(runs):
            self.rewards(ctx, references, run["symbols"][:run["steps"]], reward[s])       # :128-132
            # :134-140 -- the nll of every row (no gradient yet), summed over the loop's steps
            nll = ctx.buffer(key + ("nll", s), (run["enqueued"] * bsz,))
            ops.xent(run["logits"].data, run["symbols"].reshape(-1), None, nll)
            ops.time_sum(nll[:run["steps"] * bsz].view(1, run["steps"], bsz), logprob[s].view(1, bsz))
        ops.ew("scale", logprob.view(1, -1), None, logprob.view(1, -1), alpha=-1.0)

        row_weights = ctx.buffer(key + ("weights",), (count_s, tmax, bsz))
        scale, loss, baseline = (ctx.buffer(key + (name,), (1,)) for name in ("scale", "loss", "baseline"))
        state = {}
        if self.subtract_baseline:
            if REWARD_COUNTER not in ctx.store:
                raise RuntimeError("the session's variables were initialised before '{}' was built: they lack its "
                                   "baseline ({}, {})".format(self.name, REWARD_COUNTER, REWARD_SUM))
            state = {"reward_counter": ctx.store[REWARD_COUNTER].view(1), "reward_sum": ctx.store[REWARD_SUM].view(1)}
        ops.reinforce_sample_weights(reward, logprob, steps, row_weights, scale, loss, baseline,
                                     weight=weight / float(self.temperature), subtract_baseline=self.subtract_baseline,
                                     normalize=self.normalize, alpha=float(self.alpha), **state)
        if cost is not None:
            ops.ew("add", loss, cost, loss)
        kept_logits: List[Optional[torch.Tensor]] = [None] * count_s
        for s, run in enumerate(runs):
            if want_grad:
                F.xent(run["tape"], run["logits"], run["symbols"].reshape(-1),
                       row_weights[s, :run["enqueued"]].reshape(-1), scale)
                dec._general_backward(ctx, _Taped(run))
            else:
                kept_logits[s] = run["logits"].data.view(run["enqueued"], bsz, -1)[:run["steps"]]
        return {"loss": loss[0], "rewards": reward, "baseline": baseline[0], "sent_logprobs": logprob,
                "symbols": [run["symbols"][:run["steps"]] for run in runs], "steps": steps, "logits": kept_logits,
                "salts": [run.get("salts") for run in runs]}
    # pylint: enable=too-many-locals,protected-access

    @tensor
    def result(self, ctx) -> dict:
        """The term of this run: the trainer's (handed over with its gradients taken), or a forward pass."""
        return self.forward_backward(ctx, 1.0 if self.weight is None else float(self.weight), want_grad=False)

    @tensor
    def loss(self, ctx) -> torch.Tensor:
        return self.result(ctx)["loss"]


def rl_objective(*args, **kwargs) -> ReinforceObjective:
    """The deprecated name (rl_trainer.py:195-199)."""
    warnings.warn("Using deprecated rl_objective function. Use ReinforceObjective class directly.")
    return ReinforceObjective(*args, **kwargs)
