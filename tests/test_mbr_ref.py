"""The host oracle of MBR decoding (tests/mbr_ref.py) without a GPU: its utilities are what the reference's own
``sentence_bleu`` / ``sentence_gleu`` returned on the same tiled pairs (tests/golden/mbr/pairwise.npz, written by
tests/golden/make_mbr_golden.py), the two facts the kernel builds on -- GLEU is symmetric bit for bit with a diagonal in
{0, 1}; BLEU is not symmetric, but both of its directions have the same clipped counts -- and what the case table and
the hand-made columns are there for."""
import os

import numpy as np
import pytest

from . import mbr_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "mbr", "pairwise.npz")
NAMES = list(M.cases())


@pytest.fixture(scope="module")
def golden():
    return np.load(FIXTURE)


def test_the_fixture_holds_the_case_table(golden):
    assert sorted({k.split("/")[0] for k in golden.files}) == sorted(NAMES)
    assert NAMES[:len(M.CASES)] == [M.case_name(*c) for c in M.CASES] and len(M.CASES) == 8
    for (bsz, n, steps, words), name in zip(M.CASES, NAMES):
        tok = M.cases()[name]
        assert tok.shape == (steps, bsz, n) and tok.dtype == np.int32
        assert set(np.unique(tok)) <= {M.PAD, M.END} | set(range(3, 3 + words))
    for name in NAMES:
        tok = M.cases()[name]
        assert np.array_equal(golden[name + "/tok"], tok), name          # seeded: the table regenerates itself
        if name == "hand_made":
            continue                                                     # (its last sentence has tokens behind </s>)
        for col in tok.reshape(tok.shape[0], -1).T:                      # </s> once at most, <pad> behind it and only there
            ends = np.flatnonzero(col == M.END)
            assert len(ends) <= 1
            stop = ends[0] if len(ends) else len(col)
            assert (col[:stop] > M.END).all() and (col[stop + 1:] == M.PAD).all()
    ends = {int((M.cases()["b3_n17_t70_w5"][:, b, j] == M.END).any()) for b in range(3) for j in range(17)}
    assert ends == {0, 1}                                                # samples with and without </s>


@pytest.mark.parametrize("name", NAMES)
def test_oracle_utilities_equal_the_references(golden, name):
    bleu, gleu = M.oracle(name, "bleu").utilities, M.oracle(name, "gleu").utilities
    assert bleu.dtype == np.float32 and bleu.shape == golden[name + "/bleu"].shape
    assert bleu.tobytes() == golden[name + "/bleu"].tobytes()
    ok = golden[name + "/gleu_defined"]
    assert gleu[ok].tobytes() == golden[name + "/gleu"][ok].tobytes()
    assert np.all(gleu[~ok] == 0.0)                                      # where the reference fails its own assertion


@pytest.mark.parametrize("name", NAMES)
def test_gleu_is_symmetric_and_bleu_shares_its_counts(name):
    from neuralmonkey_amd.trainers.self_critical_objective import _ngram_counts
    gleu, bleu = M.oracle(name, "gleu").utilities, M.oracle(name, "bleu").utilities
    assert gleu.tobytes() == np.ascontiguousarray(gleu.transpose(0, 2, 1)).tobytes()
    diagonal = gleu[:, np.arange(gleu.shape[1]), np.arange(gleu.shape[1])]
    assert np.isin(diagonal, (0.0, 1.0)).all()
    tok = M.cases()[name]
    rng = np.random.default_rng(5)
    for _ in range(20):                                                  # the clipped counts of a pair, both ways round
        b, i, j = rng.integers(tok.shape[1]), rng.integers(tok.shape[2]), rng.integers(tok.shape[2])
        assert _ngram_counts(tok[:, b, i], tok[:, b, j])[0] == _ngram_counts(tok[:, b, j], tok[:, b, i])[0]
    assert ((bleu >= 0) & (bleu <= 1)).all()


def test_bleu_is_not_symmetric():
    bleu = M.oracle("b3_n17_t70_w5", "bleu").utilities
    assert not np.array_equal(bleu, bleu.transpose(0, 2, 1))
    assert (M.oracle("hand_made", "bleu").utilities[4] != M.oracle("hand_made", "bleu").utilities[4].T).any()


def test_what_the_cases_are_there_for():
    for kind in M.KINDS:
        assert M.oracle("b1_n1_t1_w3", kind).best.tolist() == [0]
        assert M.oracle("hand_empty", kind).best.tolist() == [0, 1]              # (the one word of the mix wins)
        assert not M.oracle("hand_empty", kind).expected[0].any()
        assert not M.oracle("hand_empty", kind).utilities[0].any()
        hand = M.oracle("hand_made", kind)
        assert hand.best[0] == 0 and hand.best[2] == 0 and hand.best[3] == 1
        assert hand.chosen.shape == (6, 6) and np.array_equal(hand.chosen[:, 3], M.cases()["hand_made"][:, 3, 1])
    two = M.oracle("b1_n2_t3_w3", "gleu")
    assert two.sums[0, 0] == two.sums[0, 1] and two.best.tolist() == [0]         # the tie goes to the lowest index
    hand = M.oracle("hand_made", "gleu")
    assert (hand.utilities[0] == 1.0).all() and (hand.expected[0] == 1.0).all()
    assert (hand.utilities[1] == 1.0).all()                  # </s> first: no unigram, but equal 2- to 4-grams of <pad>
    assert not M.oracle("hand_made", "bleu").utilities[1].any() and M.oracle("hand_made", "bleu").best[1] == 0
    assert hand.utilities[2, 2, 0] == 0.0 and hand.utilities[2, 2, 2] == 1.0      # the outlier shares nothing
    empty = M.oracle("b5_n8_t1_w3", "gleu")                  # T = 1: a sample is one word or </s> alone
    tok = M.cases()["b5_n8_t1_w3"][0]
    assert (tok == M.END).any() and (tok != M.END).any()
    assert not empty.utilities[tok == M.END].any()
    assert (M.oracle("b5_n3_t7_w4", "gleu").best != 0).any()                       # a choice that is not the default


def test_select_on_hand_made_utilities():
    nan = np.nan
    utilities = np.asarray([
        [[0.5, 0.5, 0.0], [0.25, 0.25, 0.5], [0.125, 0.0, 0.0]],             # top tie of rows 0 and 1: 0
        [[-3.0, -1.0, -1.0], [-1.0, -1.0, -1.0], [-2.0, -0.5, -0.5]],         # negative values: row 1 and 2 tie at -3: 1
        [[nan, 1.0, 1.0], [0.0, 0.25, 0.0], [0.0, 0.0, 0.125]],               # a NaN row sorts behind everything: 1
        [[nan, 0.0, 0.0], [0.0, nan, 0.0], [0.0, 0.0, nan]],                  # an all-NaN sentence: 0
    ], np.float32)
    tok = np.arange(2 * 4 * 3, dtype=np.int32).reshape(2, 4, 3)
    expected, best, chosen, sums = M.select(utilities, tok)
    assert best.tolist() == [0, 1, 1, 0]
    assert np.isnan(expected[2, 0]) and np.isnan(expected[3]).all() and expected[0, 0] == np.float32(1.0 / 3.0)
    assert sums[1].tolist() == [-5.0, -3.0, -3.0]
    assert chosen.tolist() == [[0, 4, 7, 9], [12, 16, 19, 21]]
