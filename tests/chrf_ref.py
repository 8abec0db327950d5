"""The rule of chrF (include/nmhip_chrf.h) restated with collections.Counter over Python strings in float64,
and the twelve-word vocabulary of the chrF tests."""
from collections import Counter
from itertools import takewhile

import numpy as np

END = 2
LONG = "ab" * 13 + "ba" * 22                             # 70 characters
# indices 4..11 behind the four special tokens: words over {a, b} of 1, 2, 3 and 70 characters, two words beyond ASCII
# (one code point each is two and three bytes of UTF-8), two BPE pieces
WORDS = ["a", "ab", "bab", LONG, "bé", "日", "ab@@", "b@@"]
A, AB, BAB, LONG_ID, E_ACUTE, KANJI, AB_GLUE, B_GLUE = range(4, 12)
SIZE = 12


def vocabulary():
    from neuralmonkey_amd.vocabulary import Vocabulary
    return Vocabulary(WORDS)


def characters(column, words, ignored=(), join_subwords=False):
    text = " ".join(words[i] for i in takewhile(lambda i: i != END and 0 <= i < len(words), column))
    return "".join(c for c in (text.replace("@@ ", "") if join_subwords else text) if c not in ignored)


def counts(ref, hyp, n):
    """int [3, 6]: matched, total_h, total_r by order, 0 above n -- the layout of nm_chrf_reward's counts."""
    out = np.zeros((3, 6), np.int32)
    for m in range(1, n + 1):
        grams_r = Counter(ref[i:i + m] for i in range(len(ref) - m + 1))
        grams_h = Counter(hyp[i:i + m] for i in range(len(hyp) - m + 1))
        out[:, m - 1] = sum((grams_r & grams_h).values()), sum(grams_h.values()), sum(grams_r.values())
    return out


def score(ref, hyp, n, beta):
    if not ref or not hyp:
        return 1.0 if ref == hyp else 0.0
    matched, total_h, total_r = counts(ref, hyp, n)[:, :n].astype(np.float64)
    precision = np.mean(np.divide(matched, total_h, out=np.ones(n), where=total_h != 0))
    recall = np.mean(np.divide(matched, total_r, out=np.ones(n), where=total_r != 0))
    if precision == 0.0 and recall == 0.0:
        return 0.0
    return (1 + beta ** 2) * precision * recall / (beta ** 2 * precision + recall)


def batch_scores(refs, hyps, words, n=6, beta=1.0, ignored=(), join_subwords=False):
    """(float64 [N], int32 [N, 3, 6]) of the time-major index arrays refs [T_ref, N], hyps [T_hyp, N]."""
    texts = [(characters(r, words, ignored, join_subwords), characters(h, words, ignored, join_subwords))
             for r, h in zip(refs.T, hyps.T)]
    return (np.array([score(r, h, n, beta) for r, h in texts]),
            np.array([counts(r, h, n) for r, h in texts]).reshape(-1, 3, 6))


# (T_hyp, T_ref, B, the pattern of column 0): between them the five batches hold every pattern where it bites
REWARD_SHAPES = [(1, 1, 3, 2), (1, 40, 5, 8), (7, 5, 7, 0), (33, 64, 5, 7), (65, 63, 3, 5)]


def _put(column, tokens):                                # the sentence, cut to the column, and </s> where there is room
    k = min(len(tokens), len(column))
    column[:k] = tokens[:k]
    if k < len(column):
        column[k] = END


def batch(t_hyp, t_ref, bsz, first):
    """Random words, and in column b the pattern (first + b) % 12: 0 no end token | 1 an empty hypothesis | 2 both empty |
    3 identical sentences | 4 no common character | 5 both sides of 1 to 5 characters | 6 the 70-character word at
    tokens 63 and 64 (or last), no end token | 7 a glued piece last in the hypothesis | 8 an index outside the table |
    9, 10, 11 streams of exactly 63, 64 and 65 characters in every column of at least 32 tokens."""
    rng = np.random.default_rng(100 * t_hyp + t_ref)
    refs = rng.integers(4, SIZE, (t_ref, bsz)).astype(np.int32)
    hyps = rng.integers(4, SIZE, (t_hyp, bsz)).astype(np.int32)
    shorter = min(t_ref, t_hyp)
    for b in range(bsz):
        pattern, ref, hyp = (first + b) % 12, refs[:, b], hyps[:, b]
        if pattern in (1, 2):
            hyp[0], ref[0] = END, END if pattern == 2 else ref[0]
        elif pattern == 3:
            hyp[:shorter] = ref[:shorter]
            if shorter > 1:
                hyp[shorter - 1] = ref[shorter - 1] = END
        elif pattern in (4, 5):
            short = [[A], [AB], [BAB], [AB, A], [AB, AB]]
            _put(hyp, [KANJI] if pattern == 4 else short[(t_hyp + b) % 5])
            _put(ref, [A] if pattern == 4 else short[(t_hyp + b + 3) % 5])
        elif pattern == 6:
            for column in (ref, hyp):
                column[[63, 64] if len(column) > 64 else [-1]] = LONG_ID
        elif pattern == 7:
            _put(hyp, list(hyp[:min(3, t_hyp - 1)]) + [AB_GLUE])
        elif pattern == 8:
            hyp[min(2, t_hyp - 1)] = SIZE + 5
            ref[min(3, t_ref - 1)] = -1
        elif pattern >= 9:
            for column in (ref, hyp):
                if len(column) >= 32:
                    _put(column, [[A], [AB], [BAB]][pattern - 9] + [A] * 31)
    return refs, hyps
