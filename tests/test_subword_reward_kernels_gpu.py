"""The reward kernel over subword pieces (csrc/nm_subword.hip, include/nmhip_subword.h) on the MI355X against what the
reference's own ``_score_with_reward_function`` returned with its GLEU and BLEU evaluators over a vocabulary of BPE
pieces (tests/golden/subword_reward/scores.npz, see make_subword_reward_golden.py).

B = 5 and B = 67 (one wavefront per sentence), (T_ref, T_hyp) = (1, 3), (7, 9) and (70, 130) -- the last runs the
segmented scan over more than one chunk of 64 positions, with words that straddle the chunks -- and the hand-made
columns of the join's corners; contiguous arrays and row strides of their own.  The tolerances and their reasons are
those of tests/test_rl_kernels_gpu.py: the kernel counts in integers and finishes in double, rounding once to float --
GLEU is a quotient of two integers, correctly rounded on both sides: EQUAL; BLEU goes through double ``log`` and
``exp``, whose last double bit may differ between the device's library and the host's, which before the one rounding
to float moves the result by at most one float32 unit in the last place.  Words are compared by (length, hash): the
generator asserts that no two distinct words of the fixture share a key, so on it the comparison is exact."""
import os

import numpy as np
import pytest
import torch

from .test_rl_kernels_gpu import SCORES as WHOLE_WORD_SCORES, ulps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORES = os.path.join(ROOT, "tests", "golden", "subword_reward", "scores.npz")
HERE = "tests/test_subword_reward_kernels_gpu.py::"
END, PAD = 2, 0
AB_, C, A_, BC, JOINER, X_, Y, ABC = range(4, 12)

pytestmark = pytest.mark.gpu

RANDOM = [(5, 1, 3), (5, 7, 9), (5, 70, 130), (67, 1, 3), (67, 7, 9), (67, 70, 130)]


class Words:
    def __init__(self, words):
        self.index_to_word = [str(w) for w in words]

    def __len__(self):
        return len(self.index_to_word)


@pytest.fixture(scope="module")
def golden():
    return np.load(SCORES)


@pytest.fixture(scope="module")
def vocab(golden):
    return Words(golden["vocabulary"])


def table_of(vocabulary):
    from neuralmonkey_amd.trainers.rl_trainer import device_piece_table
    return device_piece_table(vocabulary, "cuda:0")


def on_device(kind, ref, hyp, table, strided=False, order=4):
    from neuralmonkey_amd import ops
    dev = "cuda:0"
    if strided:                                  # rows 3 * B + 5 and 2 * B apart, the arrays in the first B columns
        bsz = ref.shape[1]
        wide_r = torch.full((ref.shape[0], 3 * bsz + 5), 4, dtype=torch.int32, device=dev)
        wide_h = torch.full((hyp.shape[0], 2 * bsz), 4, dtype=torch.int32, device=dev)
        wide_r[:, :bsz] = torch.tensor(ref, device=dev)
        wide_h[:, :bsz] = torch.tensor(hyp, device=dev)
        r, h = wide_r[:, :bsz], wide_h[:, :bsz]
        assert (ref.shape[0] == 1 or not r.is_contiguous()) and not h.is_contiguous()    # (one row is contiguous)
    else:
        r, h = torch.tensor(ref, device=dev), torch.tensor(hyp, device=dev)
    out = ops.eval_joined_sentence_score(kind, order, r, h, table)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check(name, golden, vocab):
    ref, hyp = golden[name + "/ref"], golden[name + "/hyp"]
    table = table_of(vocab)
    for strided in (False, True):
        gleu, bleu = on_device("gleu", ref, hyp, table, strided), on_device("bleu", ref, hyp, table, strided)
        print(name, "strided" if strided else "contiguous", "BLEU ulps", int(ulps(bleu, golden[name + "/bleu"]).max()),
              "GLEU ulps", int(ulps(gleu, golden[name + "/gleu"]).max()), "nonzero", int((gleu > 0).sum()), "of", gleu.size)
        assert bleu.dtype == np.float32 and gleu.dtype == np.float32
        assert np.array_equal(gleu, golden[name + "/gleu"])
        assert ulps(bleu, golden[name + "/bleu"]).max() <= 1


@pytest.mark.parametrize("bsz,t_ref,t_hyp", RANDOM)
def test_random_sentences_match_the_reference(golden, vocab, bsz, t_ref, t_hyp):
    name = "random_b{}_r{}_h{}".format(bsz, t_ref, t_hyp)
    assert golden[name + "/ref"].shape == (t_ref, bsz) and golden[name + "/hyp"].shape == (t_hyp, bsz)
    check(name, golden, vocab)


@pytest.mark.parametrize("name", ["hand_made", "hand_made_long"])
def test_hand_made_columns(golden, vocab, name):
    check(name, golden, vocab)


def test_orders_below_four_and_two_runs_are_bit_equal(golden, vocab):
    from neuralmonkey_amd.evaluators.bleu import BLEUEvaluator
    from neuralmonkey_amd.evaluators.gleu import GLEUEvaluator
    from neuralmonkey_amd.trainers.rl_trainer import score_on_the_host
    table = table_of(vocab)
    ref, hyp = golden["random_b67_r70_h130/ref"], golden["random_b67_r70_h130/hyp"]
    for kind in ("bleu", "gleu"):
        assert on_device(kind, ref, hyp, table).tobytes() == on_device(kind, ref, hyp, table).tobytes()
    for name in ("random_b67_r7_h9", "hand_made"):
        ref, hyp = golden[name + "/ref"], golden[name + "/hyp"]
        for order in (1, 2, 3):                          # the host evaluators are the reference for the orders below 4
            assert np.array_equal(on_device("gleu", ref, hyp, table, order=order),
                                  score_on_the_host(vocab, GLEUEvaluator(n=order), ref, hyp))
            assert ulps(on_device("bleu", ref, hyp, table, order=order),
                        score_on_the_host(vocab, BLEUEvaluator(n=order), ref, hyp)).max() <= 1


def test_lengths_are_bounded_and_the_longest_pair_runs(vocab):
    from neuralmonkey_amd import _lib, ops
    from neuralmonkey_amd.evaluators.gleu import GLEUEvaluator
    from neuralmonkey_amd.trainers.rl_trainer import score_on_the_host
    table = table_of(vocab)
    limit = ops.eval_joined_sentence_score_max_tokens()
    assert limit == 8192
    dev = "cuda:0"
    big = torch.full((limit, 1), C, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.NMHipError, match="above the 8192 the LDS staging holds"):
        ops.eval_joined_sentence_score("gleu", 4, big, big[:1], table)
    # the longest pair it takes, 8191 + 1 tokens: 4095 times "abc" as ab@@ c and a "y" against the one piece "abc"; ONE
    # word of 8191 continuation pieces against its first piece; "abc" behind 8190 empty prefixes against "abc"
    ref = np.zeros((limit - 1, 3), np.int32)
    ref[:, 0] = [AB_, C] * ((limit - 2) // 2) + [Y]
    ref[:, 1] = A_
    ref[:, 2] = [JOINER] * (limit - 2) + [ABC]
    hyp = np.asarray([[ABC, A_, ABC]], np.int32)
    got = ops.eval_joined_sentence_score("gleu", 4, torch.tensor(ref, device=dev), torch.tensor(hyp, device=dev), table)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    words = (limit - 2) // 2 + 1
    assert got[0] == np.float32((words - 1) / (4 * words - 6))            # recall: every "abc" of the reference's 1-grams
    assert got[1] == 0.0 and got[2] == 1.0                                 # "a" * 8190 + "a@@" is not "a@@"
    assert np.array_equal(got, score_on_the_host(vocab, GLEUEvaluator(), ref, hyp))
    # ... and the other way round: the hypothesis takes the 8191 positions
    back = ops.eval_joined_sentence_score("gleu", 4, torch.tensor(hyp, device=dev), torch.tensor(ref, device=dev), table)
    torch.cuda.synchronize()
    assert np.array_equal(back.cpu().numpy(), score_on_the_host(vocab, GLEUEvaluator(), hyp, ref))


def test_an_id_outside_the_table_cuts_the_column(golden, vocab):
    table = table_of(vocab)
    ref = golden["random_b67_r7_h9/ref"].copy()
    hyp = golden["random_b67_r7_h9/hyp"].copy()
    ref[3, ::2], hyp[4, ::3] = END, PAD
    want = on_device("gleu", ref, hyp, table)
    ref[3, ::2], hyp[4, ::3] = len(vocab), -1                             # the first id beyond the table, a negative one
    assert np.array_equal(on_device("gleu", ref, hyp, table), want)
    ref[3, ::2], hyp[4, ::3] = np.iinfo(np.int32).max, np.iinfo(np.int32).min
    assert np.array_equal(on_device("gleu", ref, hyp, table), want)


def test_whole_word_vocabulary_equals_the_index_kernel_bit_for_bit():
    """Over a vocabulary without a continuation piece every token is a word: the scores of ``ops.eval_sentence_score``."""
    from neuralmonkey_amd import ops
    from neuralmonkey_amd.trainers.rl_trainer import words_are_indices
    whole = np.load(WHOLE_WORD_SCORES)
    words = Words(whole["vocabulary"])
    assert words_are_indices(words)
    table = table_of(words)
    dev = "cuda:0"
    names = sorted({k.split("/")[0] for k in whole.files if "/" in k})
    assert len(names) == 7
    for name in names:
        ref, hyp = torch.tensor(whole[name + "/ref"], device=dev), torch.tensor(whole[name + "/hyp"], device=dev)
        for kind in ("gleu", "bleu"):
            for order in (2, 4):
                a = ops.eval_joined_sentence_score(kind, order, ref, hyp, table)
                b = ops.eval_sentence_score(kind, order, ref, hyp, END, PAD)
                torch.cuda.synchronize()
                assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), (name, kind, order)


# each entry point of include/nmhip_subword.h -> the test above that calls it (checked in tests/test_subword_reward_host.py)
LEDGER = {
    "nm_eval_joined_sentence_score_max_tokens": HERE + "test_lengths_are_bounded_and_the_longest_pair_runs via "
                                                       "ops.eval_joined_sentence_score_max_tokens",
    "nm_eval_joined_sentence_score": HERE + "test_lengths_are_bounded_and_the_longest_pair_runs via "
                                            "ops.eval_joined_sentence_score",
}
