"""Self-critical sequence training (mirror of neuralmonkey/trainers/self_critical_objective.py; Rennie et al. 2017,
https://arxiv.org/abs/1612.00563): REINFORCE on the greedy decoding with the reward of the teacher-forced (train-time)
decoding as the baseline.

    loss = -sum_{t,b} D_b * nll[t, b] * mask[t, b] / sum(mask),    D = reward(runtime) - reward(train)

with ``nll`` the negative log-likelihood of the greedy symbols under the runtime logits and ``mask`` the runtime mask;
the sign is the reference's (:85,:116-120).

MI355X mapping: the reference computes the rewards in Python behind ``tf.py_func`` -- two device-to-host read-backs and
four ``Counter`` loops per sentence and per decoding.  Here ``sentence_bleu`` and ``sentence_gleu`` are recognised by
identity and run as ONE small kernel each (csrc/nm_reward.hip: a wavefront per sentence); ``nm_reinforce_weights`` turns
rewards and mask into the row weights and the device scalars of ``nm_xent`` over the taped runtime logits, whose
gradient is written in place.  After the decoding loop the step reads nothing back.  Any other callable gets the
reference's treatment: both arrays travel to the host and the result travels back.
"""
from typing import Callable, NamedTuple

import numpy as np
import torch

from .. import autodiff as F
from .. import ops
from ..checking import check_argument_types
from ..decoders.decoder import Decoder
from ..runtime import tensor
from ..vocabulary import END_TOKEN_INDEX
from .objective import Objective

# pylint: disable=invalid-name
RewardFunction = Callable[[np.ndarray, np.ndarray], np.ndarray]
# pylint: enable=invalid-name


def _ngram_ends(seq: np.ndarray):
    """e_n for n = 1..4: the first index >= n - 1 that holds the end token, or the length."""
    ends = []
    hits = np.flatnonzero(seq == END_TOKEN_INDEX)
    for n in range(1, 5):
        later = hits[hits >= n - 1]
        ends.append(int(later[0]) if later.size else len(seq))
    return ends


def _ngram_counts(ref: np.ndarray, hyp: np.ndarray):
    """(matched_n, total_n of the hypothesis, total_n of the reference, e_1 of the reference), n = 1..4 -- integers.

    The n-grams of a sequence are its windows [i, i + n) with i + n - 1 < e_n: the window whose LAST token is the end
    token ends the list, so an end token at an index below n - 1 (which is no window's last token) ends nothing.
    ``matched`` is the clipped count: a hypothesis window matches while fewer equal hypothesis windows came before it
    than the reference holds."""
    ref_ends, hyp_ends = _ngram_ends(ref), _ngram_ends(hyp)
    matched, total_hyp, total_ref = [], [], []
    for n in range(1, 5):
        n_ref, n_hyp = max(0, ref_ends[n - 1] - n + 1), max(0, hyp_ends[n - 1] - n + 1)
        budget = {}
        for i in range(n_ref):
            key = tuple(int(t) for t in ref[i:i + n])
            budget[key] = budget.get(key, 0) + 1
        hits = 0
        for i in range(n_hyp):
            key = tuple(int(t) for t in hyp[i:i + n])
            if budget.get(key, 0) > 0:
                budget[key] -= 1
                hits += 1
        matched.append(hits)
        total_hyp.append(n_hyp)
        total_ref.append(n_ref)
    return matched, total_hyp, total_ref, ref_ends[0]


def sentence_bleu(references: np.ndarray, hypotheses: np.ndarray) -> np.ndarray:
    """Index-based sentence-level BLEU of time-major ``references`` [T_ref, B] and ``hypotheses`` [T_hyp, B]: whatever
    the decoder emits is a token.  Orders above 1 are smoothed by one matched and one counted n-gram; a hypothesis
    without a unigram scores 0."""
    scores = []
    for ref, hyp in zip(np.transpose(references), np.transpose(hypotheses)):
        matched, total, _, ref_len = _ngram_counts(ref, hyp)
        if total[0] == 0:
            scores.append(0.0)
            continue
        hit, seen = matched[0], total[0]
        for n in range(1, 4):
            hit *= matched[n] + 1
            seen *= total[n] + 1
        precision = (np.float64(hit) / np.float64(seen)) ** .25
        brevity = np.min([1., np.exp(1 - ref_len / total[0])])
        scores.append(brevity * precision)
    return np.array(scores, dtype=np.float32)


def sentence_gleu(references: np.ndarray, hypotheses: np.ndarray) -> np.ndarray:
    """Index-based GLEU (https://arxiv.org/abs/1609.08144): the minimum of precision and recall over the 1- to 4-grams;
    0 where either side has no n-gram at all (the reference fails its own assertion there)."""
    scores = []
    for ref, hyp in zip(np.transpose(references), np.transpose(hypotheses)):
        matched, total_hyp, total_ref, _ = _ngram_counts(ref, hyp)
        hit, n_hyp, n_ref = sum(matched), sum(total_hyp), sum(total_ref)
        if n_hyp == 0 or n_ref == 0:
            scores.append(0.0)
        else:
            scores.append(min(np.float64(hit) / np.float64(n_hyp), np.float64(hit) / np.float64(n_ref)))
    return np.array(scores, dtype=np.float32)


# the reward functions that run on the device: function -> ops.sentence_reward kind
DEVICE_REWARDS = {sentence_bleu: "bleu", sentence_gleu: "gleu"}


class _Taped(NamedTuple):
    """What ``Decoder._general_backward`` reads of a train result."""
    saved: dict


class SelfCriticalObjective(Objective):
    """self_critical_objective.py:28-92.  ``reward_function`` maps time-major (references [T_ref, B], hypotheses
    [T_hyp, B]) to one float32 per sentence; ``sentence_bleu`` and ``sentence_gleu`` of this module run on the device."""

    def __init__(self, decoder: Decoder, reward_function: RewardFunction, weight: float = None) -> None:
        check_argument_types()
        Objective.__init__(self, "{}_self_critical".format(decoder.name), decoder)
        self.reward_function = reward_function
        self.weight = weight

    # -- rewards ------------------------------------------------------------------------------------------------
    def rewards(self, ctx, references: torch.Tensor, hypotheses: torch.Tensor, tag: str) -> torch.Tensor:
        """[B] float32 on the device.  The two functions of this module: one kernel launch.  Anything else: the
        reference's ``tf.py_func`` -- both arrays to the host (a synchronisation), the result back."""
        bsz = references.shape[1]
        out = ctx.buffer((id(self), "reward", tag, bsz), (bsz,))
        kind = DEVICE_REWARDS.get(self.reward_function)
        if kind is not None and references.is_cuda:
            return ops.sentence_reward(kind, references, hypotheses, END_TOKEN_INDEX, out=out)
        host = self.reward_function(references.cpu().numpy(), hypotheses.cpu().numpy().astype(np.int64))
        host = np.ascontiguousarray(np.asarray(host, dtype=np.float32).reshape(bsz))
        return out.copy_(torch.from_numpy(host))

    # -- the term ------------------------------------------------------------------------------------------------
    def forward_backward(self, ctx, weight: float, want_grad: bool = True) -> dict:
        """The taped greedy loop, both rewards, the loss and -- with ``want_grad`` -- its gradient: into the flat
        gradient buffer (accumulated) and, through ``ctx.defer_backward``, into the encoders.  The train-time
        hypotheses are those of the teacher-forced pass this context has run (a cost objective over the same decoder:
        ``want_train_argmax`` was set before it ran); without one a pass of its own runs, without gradient."""
        dec = self.decoder
        if (id(dec), "train_argmax") not in ctx.memo:
            ctx.memo[(id(dec), "want_train_argmax")] = True
            dec._train_loop(ctx, want_grad=False)                      # pylint: disable=protected-access
        train_hyp = ctx.memo[(id(dec), "train_argmax")]
        run = dec.taped_runtime_loop(ctx, record=want_grad)
        steps, enqueued, bsz = run["steps"], run["enqueued"], run["bsz"]
        references = dec.train_inputs(ctx)
        runtime_hyp = run["argmax"][:steps]          # tf.argmax(runtime_logits, axis=2): the loop's length, raw argmax
        reward = self.rewards(ctx, references, runtime_hyp, "runtime")
        baseline = self.rewards(ctx, references, train_hyp, "train")

        key = (id(self), "term", enqueued, bsz)
        row_weights = ctx.buffer(key + ("weights",), (enqueued, bsz))
        scale, inv_count = ctx.buffer(key + ("scale",), (1,)), ctx.buffer(key + ("inv",), (1,))
        ops.reinforce_weights(reward, baseline, run["mask"], weight, row_weights, scale, inv_count)
        loss_rows = F.xent(run["tape"], run["logits"], run["argmax"].reshape(-1), row_weights.view(-1), scale)
        loss_sum, loss = ctx.buffer(key + ("loss_sum",), (1,)), ctx.buffer(key + ("loss",), (1,))
        ops.reduce_sum(loss_rows, loss_sum)
        ops.ew("mul", loss_sum, inv_count, loss)
        if want_grad:
            dec._general_backward(ctx, _Taped(run))                    # pylint: disable=protected-access
        return {"loss": loss[0], "reward": reward, "baseline": baseline, "train_argmax": train_hyp,
                "runtime_argmax": runtime_hyp, "mask": run["mask"][:steps], "symbols": run["symbols"][:steps],
                "steps": steps}

    @tensor
    def result(self, ctx) -> dict:
        """The term of this run: the trainer's (handed over with its gradients taken), or a forward pass."""
        return self.forward_backward(ctx, 1.0 if self.weight is None else float(self.weight), want_grad=False)

    @tensor
    def loss(self, ctx) -> torch.Tensor:
        return self.result(ctx)["loss"]


def reinforce_score(reward: torch.Tensor, baseline: torch.Tensor, decoded: torch.Tensor,
                    logits: torch.Tensor) -> torch.Tensor:
    """self_critical_objective.py:95-121: (reward - baseline)[None, :] * nll of ``decoded`` [T, B] under ``logits``
    [T, B, V], whose derivative with respect to the logits is the REINFORCE update; reward and baseline are constants
    of it.  A plain torch expression for callers outside the trainer -- the objective itself runs ``nm_xent`` with the
    weights of ``nm_reinforce_weights``."""
    steps, bsz, vocab = logits.shape
    nll = torch.nn.functional.cross_entropy(logits.reshape(steps * bsz, vocab), decoded.reshape(-1).long(),
                                            reduction="none").view(steps, bsz)
    return (reward - baseline).detach().unsqueeze(0) * nll
