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
gradient is written in place.  After the decoding loop the step reads nothing back.  ``sentence_edit_accuracy`` and
``sentence_neg_wer`` (minimum-WER training; the rule is this project's) are recognised the same way and run
as one launch of csrc/nm_edit.hip; a ``SentenceChrF`` object (the reference's chrF over the characters of the tokens'
words) as one launch of csrc/nm_chrf.hip.  Any other callable gets the reference's treatment: both arrays
travel to the host and the result travels back.
"""
from typing import Callable, Dict, List, NamedTuple

import numpy as np
import torch

from .. import autodiff as F
from .. import ops
from ..checking import check_argument_types
from ..decoders.decoder import Decoder
from ..runtime import tensor
from ..vocabulary import END_TOKEN_INDEX, Vocabulary
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


def _edit_counts(ref: np.ndarray, hyp: np.ndarray):
    """(d, lr, lh): the Levenshtein distance of the two sentences ``seq[:e_1]`` and their lengths -- integers.

    Row ``i`` of the table from row ``i - 1``: ``open[j] = min(up + 1, diagonal + (tokens differ))`` for all ``j`` at
    once; the chain through the left neighbour, ``row[j] = min(open[j], row[j - 1] + 1)``, is a running minimum of
    ``open[j] - j``."""
    lr, lh = _ngram_ends(ref)[0], _ngram_ends(hyp)[0]
    hyp, columns = np.asarray(hyp[:lh]), np.arange(lh + 1)
    row = columns.copy()
    for i in range(lr):
        opened = np.concatenate(([i + 1], np.minimum(row[1:] + 1, row[:-1] + (hyp != ref[i]))))
        row = np.minimum.accumulate(opened - columns) + columns
    return int(row[lh]), lr, lh


def sentence_edit_accuracy(references: np.ndarray, hypotheses: np.ndarray) -> np.ndarray:
    """``1 - d / max(lr, lh)`` of time-major ``references`` [T_ref, B] and ``hypotheses`` [T_hyp, B], ``d`` the
    Levenshtein distance over token indices of the two sentences, each cut at its first end token (whatever else the
    decoder emitted is a token), ``lr`` and ``lh`` their lengths; 1 when both are empty.  Symmetric, in [0, 1]: the
    character or word accuracy of speech recognition as a sentence-level utility."""
    scores = []
    for ref, hyp in zip(np.transpose(references), np.transpose(hypotheses)):
        dist, n_ref, n_hyp = _edit_counts(ref, hyp)
        longer = max(n_ref, n_hyp)
        scores.append(1.0 if longer == 0 else 1.0 - np.float64(dist) / np.float64(longer))
    return np.array(scores, dtype=np.float32)


def sentence_neg_wer(references: np.ndarray, hypotheses: np.ndarray) -> np.ndarray:
    """``-d / max(lr, 1)``: the negative word error rate of every sentence, the reward of minimum-WER training."""
    scores = []
    for ref, hyp in zip(np.transpose(references), np.transpose(hypotheses)):
        dist, n_ref, _ = _edit_counts(ref, hyp)
        scores.append(np.float64(-dist) / np.float64(max(n_ref, 1)))
    return np.array(scores, dtype=np.float32)


# the reward functions that run on the device: function -> ops.sentence_reward kind
DEVICE_REWARDS = {sentence_bleu: "bleu", sentence_gleu: "gleu"}
# ... and those of csrc/nm_edit.hip: function -> ops.edit_reward / ops.edit_pairwise kind, for columns of at most
# ops.edit_max_tokens() positions
DEVICE_EDIT_REWARDS = {sentence_edit_accuracy: "accuracy", sentence_neg_wer: "neg_wer"}

CHRF_GLUE, CHRF_SPACE_DROPPED = 1, 2                     # the flags of a character-table row (include/nmhip_chrf.h)
CHRF_SPACE_ID, CHRF_MAX_ORDER, CHRF_MAX_CHARACTERS = 0, 6, 65534


def _char_ngrams(chars: List[str], n: int) -> List[Dict[str, int]]:
    """evaluators/chrf.py:89-97: per order m = 1..n the counts of the m-grams of ``chars``, keyed by their text."""
    orders = []
    for m in range(1, n + 1):
        counted = {}  # type: Dict[str, int]
        for i in range(len(chars) - m + 1):
            gram = "".join(chars[i:i + m])
            counted[gram] = counted.get(gram, 0) + 1
        orders.append(counted)
    return orders


class SentenceChrF:
    """chrF (http://www.statmt.org/wmt15/pdf/WMT49.pdf) of time-major index arrays, the reference's
    ``ChrFEvaluator.score_instance`` (evaluators/chrf.py:35-97) per sentence: a ``reward_function`` of
    ``SelfCriticalObjective`` and a ``utility`` of ``MBRDecoder``, which recognise the class and score on the device
    from ``device_table`` (csrc/nm_chrf.hip).  ``n``, ``beta`` and ``ignored_symbols`` default as the
    reference's do; ``beta=3`` is its ``ChrF3``.  Orders above 6 are not offered.

    The sentence of a column is its tokens before the first ``</s>`` index or index outside the vocabulary; its text is
    their words joined by spaces -- with ``join_subwords`` after the reference's BPE join, ``.replace("@@ ", "")`` --;
    its characters are the text's code points without ``ignored_symbols``.  Calling the object is the host statement
    of the rule, and the route of CPU tensors."""

    def __init__(self, vocabulary: Vocabulary, n: int = 6, beta: float = 1.0, ignored_symbols: List[str] = None,
                 join_subwords: bool = False) -> None:
        check_argument_types()
        if not 1 <= n <= CHRF_MAX_ORDER:
            raise ValueError("SentenceChrF: n = {} outside 1..{}".format(n, CHRF_MAX_ORDER))
        if not beta > 0:
            raise ValueError("SentenceChrF: beta = {} is not above 0".format(beta))
        self.vocabulary = vocabulary
        self.n = n
        self.beta = float(beta)
        self.ignored = frozenset(ignored_symbols or ())
        self.join_subwords = join_subwords
        self.table()                                     # ValueError for a vocabulary the table cannot hold

    # -- the rule, on the host ----------------------------------------------------------------------------------
    def characters(self, column) -> List[str]:
        words = self.vocabulary.index_to_word
        kept = []
        for index in column:
            if index == END_TOKEN_INDEX or not 0 <= index < len(words):
                break
            kept.append(words[index])
        text = " ".join(kept)
        if self.join_subwords:
            text = text.replace("@@ ", "")
        return [c for c in text if c not in self.ignored]

    def counts(self, ref_chars: List[str], hyp_chars: List[str]):
        """(matched, total_h, total_r), each a list over the orders 1..n -- integers."""
        ref_grams, hyp_grams = _char_ngrams(ref_chars, self.n), _char_ngrams(hyp_chars, self.n)
        matched = [sum(min(count, ref[gram]) for gram, count in hyp.items() if gram in ref)
                   for ref, hyp in zip(ref_grams, hyp_grams)]
        return (matched, [max(0, len(hyp_chars) - m) for m in range(self.n)],
                [max(0, len(ref_chars) - m) for m in range(self.n)])

    def score(self, ref_chars: List[str], hyp_chars: List[str]) -> float:
        if not ref_chars or not hyp_chars:
            return 1.0 if not ref_chars and not hyp_chars else 0.0
        matched, total_h, total_r = self.counts(ref_chars, hyp_chars)
        precision = recall = 0.0
        for hit, n_hyp, n_ref in zip(matched, total_h, total_r):
            precision += hit / n_hyp if n_hyp else 1.0
            recall += hit / n_ref if n_ref else 1.0
        precision /= self.n
        recall /= self.n
        if precision == 0.0 and recall == 0.0:
            return 0.0
        beta_2 = self.beta * self.beta
        return (1.0 + beta_2) * (precision * recall) / (beta_2 * precision + recall)

    def __call__(self, references: np.ndarray, hypotheses: np.ndarray) -> np.ndarray:
        scores = [self.score(self.characters(ref), self.characters(hyp))
                  for ref, hyp in zip(np.transpose(references), np.transpose(hypotheses))]
        return np.array(scores, dtype=np.float32)

    # -- the character table ------------------------------------------------------------------------------------
    def table(self):
        """(rows int32 [V, 4], chars uint16 [total], max_word_chars) of include/nmhip_chrf.h: per word (offset,
        stem_len, whole_len, flags) into the dense ids of its kept characters, the stem -- the text without a trailing
        "@@" -- first; id 0 is the space.  Computed once per (vocabulary, ignored symbols, join) and kept on the
        vocabulary, with its device copies."""
        cache = self.vocabulary.__dict__.setdefault("_chrf_tables", {})
        key = (tuple(sorted(self.ignored)), self.join_subwords)
        if key not in cache or cache[key][0] != len(self.vocabulary):
            words = list(self.vocabulary.index_to_word)
            if not all(w and " " not in w for w in words):
                raise ValueError("SentenceChrF: the vocabulary has an empty word or a word with a space")
            ids = {" ": CHRF_SPACE_ID}
            rows, chars = np.zeros((len(words), 4), np.int32), []
            dropped = CHRF_SPACE_DROPPED if " " in self.ignored else 0
            for row, word in zip(rows, words):
                glue = self.join_subwords and word.endswith("@@")
                stem = [c for c in (word[:-2] if glue else word) if c not in self.ignored]
                tail = [c for c in "@@" if c not in self.ignored] if glue else []
                row[:] = (len(chars), len(stem), len(stem) + len(tail), (CHRF_GLUE if glue else 0) | dropped)
                chars.extend(ids.setdefault(c, len(ids)) for c in stem + tail)
            if len(ids) > CHRF_MAX_CHARACTERS:
                raise ValueError("SentenceChrF: {} distinct characters, the space included, are more than {}"
                                 .format(len(ids), CHRF_MAX_CHARACTERS))
            cache[key] = (len(words), rows, np.array(chars or [CHRF_SPACE_ID], np.uint16),
                          max(1, int(rows[:, 2].max())), {})
        return cache[key][1:4]

    def device_table(self, device) -> ops.CharTable:
        """``table`` on ``device``, copied there once per device."""
        rows, chars, max_word_chars = self.table()
        on_devices = self.vocabulary.__dict__["_chrf_tables"][(tuple(sorted(self.ignored)), self.join_subwords)][4]
        name = str(torch.device(device))
        if name not in on_devices:
            on_devices[name] = ops.CharTable(torch.from_numpy(rows).to(device),
                                             torch.from_numpy(chars.view(np.int16)).to(device), max_word_chars)
        return on_devices[name]

    def on_device(self, tokens: int) -> bool:
        """Whether columns of ``tokens`` positions together fit the kernels' static bound."""
        return tokens * (self.table()[2] + 1) <= ops.chrf_max_chars()


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
        """[B] float32 on the device.  The four functions of this module: one kernel launch (the two edit-distance
        ones up to ``ops.edit_max_tokens()`` positions); so is a ``SentenceChrF`` while its static bound fits
        ``ops.chrf_max_chars()``.  Anything else: the reference's ``tf.py_func`` -- both arrays to the host (a
        synchronisation), the result back."""
        bsz = references.shape[1]
        out = ctx.buffer((id(self), "reward", tag, bsz), (bsz,))
        kind = DEVICE_REWARDS.get(self.reward_function)
        if kind is not None and references.is_cuda:
            return ops.sentence_reward(kind, references, hypotheses, END_TOKEN_INDEX, out=out)
        kind = DEVICE_EDIT_REWARDS.get(self.reward_function)
        if (kind is not None and references.is_cuda
                and max(references.shape[0], hypotheses.shape[0]) <= ops.edit_max_tokens()):
            return ops.edit_reward(kind, references, hypotheses, END_TOKEN_INDEX, out=out)
        chrf = self.reward_function
        if (isinstance(chrf, SentenceChrF) and references.is_cuda
                and chrf.on_device(references.shape[0] + hypotheses.shape[0])):
            return ops.chrf_reward(references, hypotheses, END_TOKEN_INDEX, chrf.device_table(references.device),
                                   chrf.n, chrf.beta, out=out)
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
